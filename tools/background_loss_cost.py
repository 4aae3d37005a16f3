"""Dev probe (GPU): the loss phase of NativeTrainStep (`_loss`: the fused HIP loss where it applies, else image-sized torch autograd)
at 1237x822 for model.background.color black, white and random, under device events.  `--tree DIR` imports the package from another
checkout (one built there), so the same probe times an older commit — where `random` still takes the torch branch — beside this one:
run the two alternately and compare the medians against the spread between repeats of one tree.

Two figures per colour, from `--samples` samples each after `--warmup` calls: `single` = one call between two events (includes
the host's launch gaps when the host is the slower side, as in the torch branch), `queued` = `--burst` calls between two events
over `--burst` (the device's own time per call once the queue is full, which is what the step's critical path sees).

    python tools/background_loss_cost.py [--tree DIR] [--samples 60] [--burst 20] [--warmup 20] [--masked]
"""
import argparse
import importlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--width", type=int, default=1237)
    ap.add_argument("--height", type=int, default=822)
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--masked", action="store_true", help="give the batch a mask (left third zero)")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    if not torch.cuda.is_available():
        raise SystemExit("background_loss_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    g = torch.Generator().manual_seed(0)
    rgba = torch.rand((H, W, 4), generator=g).to(dev)                 # a stand-in for the render: the loss kernels' time does not
    gt = torch.rand((1, H, W, 3), generator=g).to(dev)                # depend on the values
    ro, rd = cams.pinhole_rays(W, H, 0.9 * W, 0.9 * W)
    batch = gut.Batch(rays_ori=torch.as_tensor(ro, device=dev), rays_dir=torch.as_tensor(rd, device=dev),
                      T_to_world=torch.eye(4, device=dev)[None], rgb_gt=gt,
                      intrinsics_OpenCVPinholeCameraModelParameters=cams.pinhole_intrinsics_dict(W, H, 0.9 * W, 0.9 * W))
    if a.masked:
        mask = torch.ones((1, H, W, 1), dtype=torch.float32, device=dev)
        mask[:, :, :W // 3] = 0.0
        batch.mask = mask
    tracer = gut.Tracer({"render": {}})
    out = {"label": a.label, "tree": os.path.abspath(a.tree), "size": [W, H], "masked": bool(a.masked), "samples": a.samples,
           "burst": a.burst}

    def timed(st, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            st._loss(batch, rgba)
        e1.record()
        return e0, e1

    def stats(pairs, calls):
        t = sorted(x.elapsed_time(y) / calls for x, y in pairs)
        return dict(median_ms=round(t[len(t) // 2], 5), p10_ms=round(t[len(t) // 10], 5), p90_ms=round(t[(9 * len(t)) // 10], 5),
                    min_ms=round(t[0], 5))

    steppers = {}
    for color in ("black", "white", "random"):
        model = native.NativeGaussianModel(scenes.scene_c1(1000, 1), device=dev, background_color=color)
        steppers[color] = native.NativeTrainStep(model, tracer, scene_extent=1.0)
    for rnd in range(2):                                               # two rounds, the colours alternating: the spread between
        for color, st in steppers.items():                             # rounds is the noise to read a difference against
            for _ in range(a.warmup):
                st._loss(batch, rgba)
            torch.cuda.synchronize()
            single = [timed(st, 1) for _ in range(a.samples)]
            torch.cuda.synchronize()
            queued = [timed(st, a.burst) for _ in range(a.samples)]
            torch.cuda.synchronize()
            res = dict(single=stats(single, 1), queued=stats(queued, a.burst))
            out[f"{color}_round{rnd}"] = res
            print(f"[{a.label or 'tree'}] {color} round {rnd}: single median {res['single']['median_ms']:.4f} ms "
                  f"(p10 {res['single']['p10_ms']:.4f}, p90 {res['single']['p90_ms']:.4f}); queued median "
                  f"{res['queued']['median_ms']:.4f} ms (p10 {res['queued']['p10_ms']:.4f}, p90 {res['queued']['p90_ms']:.4f})", flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
