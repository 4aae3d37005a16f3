"""Dev probe (GPU): what the affine form of the fused loss (gut_photometric_loss_exposure: the kExposure forward and backward, the
per-pixel pass k_exposure_grad for every background, k_exposure_finish) and the twelve-float Adam cost.

Part 1, the step: one NativeTrainStep(exposure_gradient=True) on a bench workload's scene, built as bench.py builds it (Morton-ordered
rows, synthetic mid-training optimiser state, placement tuned); blocks of `--block` steps alternate between batches without an
exposure (the existing form, launch for launch) and batches with one followed by ExposureCompensation.end, `--rounds` times, each
block timed event to event and by phase (phase_times_mean: the loss phase is the figure).
Part 2, the loss alone: `_loss` at the workload's image size for black, white and random backgrounds, without an exposure, with one
applied only (no reduction) and with the reduction, `--burst` calls between two events (the device's own time per call).

    python tools/exposure_cost.py [--workload bicycle_like_6M_1237x822] [--block 24] [--rounds 4] [--warmup 16] [--skip-step]
"""
import argparse
import copy
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle_like_6M_1237x822")
    ap.add_argument("--num-gaussians", type=int, default=0)
    ap.add_argument("--block", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--skip-step", action="store_true", help="part 2 only")
    a = ap.parse_args()
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    exposure = importlib.import_module("3dgrut_amd.exposure")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    if not torch.cuda.is_available():
        raise SystemExit("exposure_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[a.workload]
    kw = dict(kw)
    if a.num_gaussians:
        kw["n"] = a.num_gaussians
    n_views = 8
    ro, rd, c2ws = bench.make_views(cams, n_views, W, H, fx, radius, elev, False)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(100)).to(dev)
    batches = [gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[v])[None], rgb_gt=gt,
                         intrinsics_OpenCVPinholeCameraModelParameters=K) for v in range(n_views)]
    tracer = gut.Tracer({"render": {}})
    report = dict(workload=a.workload, size=[W, H])

    if not a.skip_step:
        scene = getattr(scenes, fn)(**kw)
        model = native.NativeGaussianModel(scene, device=dev, sh_degree=3, spatial_order=True)
        st = native.NativeTrainStep(model, tracer, scene_extent=extent, exposure_gradient=True)
        bench.synthetic_optimizer_state(st)
        comp = exposure.ExposureCompensation(n_views, dev)
        step = 0

        def one(on):
            nonlocal step
            v = step % n_views
            st.step(comp.begin(v, batches[v]) if on else batches[v])
            if on:
                comp.end(v, st.exposure_gradient)
            step += 1

        for s in range(a.warmup):
            one(False)
            if s == 1 and model.num_gaussians >= 1_000_000:
                st.tune_placement()
        while st.probe_pending and step < a.warmup + 16:
            torch.cuda.synchronize()
            one(False)
        torch.cuda.synchronize()
        st.phase_timing = True
        results = {"off": [], "on": []}
        for rnd in range(a.rounds):
            for on in (False, True):
                for _ in range(4):                       # settle after the switch
                    one(on)
                torch.cuda.synchronize()
                st.phase_times_mean()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.block):
                    one(on)
                e1.record()
                torch.cuda.synchronize()
                phases = st.phase_times_mean()
                rec = dict(step_ms=round(e0.elapsed_time(e1) / a.block, 4), **{k: round(v, 4) for k, v in phases.items()})
                results["on" if on else "off"].append(rec)
                print(f"[exposure cost] round {rnd} {'on ' if on else 'off'}: {json.dumps(rec)}", flush=True)
        report["step_median"] = {key: {k: round(sorted(r[k] for r in recs)[len(recs) // 2], 4) for k in recs[0]}
                                 for key, recs in results.items()}
        report["n"] = model.num_gaussians
        report["mean_gain_after"] = comp.summary()["mean_gain"]
        del st, model, scene
        torch.cuda.empty_cache()

    rgba = torch.rand((H, W, 4), generator=torch.Generator().manual_seed(0)).to(dev)   # the loss kernels' time does not depend on values
    E = torch.tensor(exposure.IDENTITY, dtype=torch.float32, device=dev)
    with_e = copy.copy(batches[0])
    with_e.exposure = E

    def queued(st, batch):
        for _ in range(a.burst):
            st._loss(batch, rgba)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.burst):
                st._loss(batch, rgba)
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / a.burst)
        t.sort()
        return round(t[len(t) // 2], 5)

    loss_only = {}
    for color in ("black", "white", "random"):
        model = native.NativeGaussianModel(scenes.scene_c1(1000, 1), device=dev, background_color=color)
        st = native.NativeTrainStep(model, tracer, scene_extent=1.0, exposure_gradient=True)
        for rnd in range(2):
            rec = dict(none=queued(st, batches[0]))
            st.enable_exposure_gradient(False)
            rec["applied"] = queued(st, with_e)
            st.enable_exposure_gradient(True)
            rec["reduced"] = queued(st, with_e)
            loss_only[f"{color}_round{rnd}"] = rec
            print(f"[exposure cost] loss alone, {color}, round {rnd}: {json.dumps(rec)} ms per call", flush=True)
    report["loss_only_ms"] = loss_only
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
