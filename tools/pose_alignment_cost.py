"""Dev probe (GPU): what one iteration of the held-out pose alignment (pose_align.PoseAligner) costs on a bench
workload, split into forward / loss / backward, with the Gaussians frozen:

  (a) the pose-only backward (gut_trace_bwd_pose: the compositor and the consuming reduction, no epilogue);
  (b) the plain gut_trace_bwd with dense [N,12] + [N,48] outputs while the pose output is set: the only way to the same eight floats
      before the pose-only backward existed (the outputs are allocated once, outside the timed region).

Blocks of `--block` iterations alternate between the two, `--rounds` times; every phase is timed event to event and an iteration ends
with the synchronisation the aligner has.  `--consume store` runs the consuming reduction in its other form (GUT_POSE_CONSUME=store: four
unconditional zero stores per visited row) instead of the default, which reads the whole row and stores only where a word is set; run
the tool once with each to compare them.

    python tools/pose_alignment_cost.py [--workload bicycle_like_6M_1237x822] [--block 24] [--rounds 3] [--consume test|store]
"""
import argparse
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--consume", choices=("test", "store"), default="test")
    a = ap.parse_args()
    if a.consume == "store":
        os.environ["GUT_POSE_CONSUME"] = "store"     # read by the library at its first pose-only backward
    else:
        os.environ.pop("GUT_POSE_CONSUME", None)
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    pose_align = importlib.import_module("3dgrut_amd.pose_align")
    if not torch.cuda.is_available():
        raise SystemExit("pose_alignment_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[a.workload]
    kw = dict(kw)
    if a.num_gaussians:
        kw["n"] = a.num_gaussians
    scene = getattr(scenes, fn)(**kw)
    tracer = gut.Tracer({"render": {}})
    model = native.NativeGaussianModel(scene, device=dev, sh_degree=3, spatial_order=True)
    n = model.num_gaussians
    n_views = 8
    ro, rd, c2ws = bench.make_views(cams, n_views, W, H, fx, radius, elev, False)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(100)).to(dev)
    batches = [gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[v])[None], rgb_gt=gt,
                         intrinsics_OpenCVPinholeCameraModelParameters=K) for v in range(n_views)]
    step = pose_align.DeviceStep(model, tracer)
    step.acquire()
    raster = step.raster
    dense = (torch.empty((n, 12), device=dev), torch.empty((n, 48), device=dev))

    def iteration(view, pose_only, evs=None):
        mark = (lambda: None) if evs is None else (lambda: (evs.append(torch.cuda.Event(enable_timing=True)), evs[-1].record()))
        mark()
        sensor, poses = step._create_camera(batches[view])
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        rgba, dist, _, _ = raster.trace(0, 3, step.act, step.features, ro_t, rd_t, None, *cam)
        mark()
        loss3, rgba_grad = pose_align_loss(step, batches[view], rgba)
        mark()
        if pose_only:
            raster.trace_bwd_pose(0, 3, step.act, ro_t, rd_t, *cam, rgba, rgba_grad, dist, None)
        else:
            raster.trace_bwd(0, 3, step.act, step.features, ro_t, rd_t, None, *cam, rgba, rgba_grad, dist, None, out=dense)
        mark()
        torch.cuda.synchronize()

    it = 0
    for _ in range(a.warmup):
        for mode in (True, False):
            iteration(it % n_views, mode); it += 1
    results = {"pose_only": [], "dense": []}
    for rnd in range(a.rounds):
        for mode in (True, False):
            for _ in range(2):                       # settle after the switch
                iteration(it % n_views, mode); it += 1
            acc = [0.0, 0.0, 0.0]
            for _ in range(a.block):
                evs = []
                iteration(it % n_views, mode, evs); it += 1
                for k in range(3):
                    acc[k] += evs[k].elapsed_time(evs[k + 1])
            rec = dict(forward=round(acc[0] / a.block, 4), loss=round(acc[1] / a.block, 4), backward=round(acc[2] / a.block, 4))
            rec["iteration_ms"] = round(sum(acc) / a.block, 4)
            results["pose_only" if mode else "dense"].append(rec)
            print(f"[alignment cost] round {rnd} {'pose-only' if mode else 'dense    '}: {json.dumps(rec)}", flush=True)
    out8 = [float(x) for x in step.out8.tolist()]
    step.release()
    summary = {key: {k: round(sorted(r[k] for r in recs)[len(recs) // 2], 4) for k in recs[0]} for key, recs in results.items()}
    print(json.dumps(dict(workload=a.workload, n=n, consume=a.consume, block=a.block, rounds=a.rounds, median=summary, pose_gradient=out8)), flush=True)


def pose_align_loss(step, batch, rgba):
    """The fused loss of DeviceStep.forward_loss on an rgba that is already rendered."""
    losses = importlib.import_module("3dgrut_amd.losses")
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    need = step._lib.gut_photometric_workspace_bytes(H, W)
    if step._ws is None or step._ws.numel() * 4 < need:
        import torch
        step._ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=rgba.device)
    return losses._photometric_loss_call(step._lib, H, W, rgba, batch.rgb_gt, step.background, step.lambda_l1, step.lambda_ssim, None, step._ws)


if __name__ == "__main__":
    main()
