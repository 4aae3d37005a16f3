"""Dev probe (GPU): what a learnt environment map (gut_environment_sample before the loss, gut_environment_backward
and the map's Adam step behind it) costs a train step of a bench workload.  One NativeTrainStep on the workload's scene, built as
bench.py builds it (Morton-ordered rows, synthetic mid-training optimiser state, placement tuned); blocks of `--block` steps
alternate between model.environment None and the map, `--rounds` times, each block timed event to event and by phase
(phase_times_mean).

    python tools/environment_cost.py [--workload bicycle_like_6M_1237x822] [--resolution 256] [--block 24] [--rounds 4] [--warmup 16]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/environment_cost.py --rounds 1 --only-on     # the four kernels' own times
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
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--block", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--only-on", action="store_true", help="every block with the map on (profiler runs)")
    a = ap.parse_args()
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    environment = importlib.import_module("3dgrut_amd.environment")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    if not torch.cuda.is_available():
        raise SystemExit("environment_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[a.workload]
    kw = dict(kw)
    if a.num_gaussians:
        kw["n"] = a.num_gaussians
    scene = getattr(scenes, fn)(**kw)
    tracer = gut.Tracer({"render": {}})
    model = native.NativeGaussianModel(scene, device=dev, sh_degree=3, spatial_order=True)
    st = native.NativeTrainStep(model, tracer, scene_extent=extent)
    bench.synthetic_optimizer_state(st)
    env = environment.EnvironmentMap(a.resolution, 0.5, dev)
    n_views = 8
    ro, rd, c2ws = bench.make_views(cams, n_views, W, H, fx, radius, elev, False)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(100)).to(dev)
    batches = [gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[v])[None], rgb_gt=gt,
                         intrinsics_OpenCVPinholeCameraModelParameters=K) for v in range(n_views)]

    step = 0
    for s in range(a.warmup):
        st.step(batches[step % n_views]); step += 1
        if s == 1 and model.num_gaussians >= 1_000_000:
            st.tune_placement()
    while st.probe_pending and step < a.warmup + 16:
        torch.cuda.synchronize()
        st.step(batches[step % n_views]); step += 1
    torch.cuda.synchronize()
    st.phase_timing = True
    results = {"off": [], "on": []}
    for rnd in range(a.rounds):
        for on in ((True,) if a.only_on else (False, True)):
            model.environment = env if on else None
            for _ in range(4):                       # settle after the switch
                st.step(batches[step % n_views]); step += 1
            torch.cuda.synchronize()
            st.phase_times_mean()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.block):
                st.step(batches[step % n_views]); step += 1
            e1.record()
            torch.cuda.synchronize()
            phases = st.phase_times_mean()
            rec = dict(step_ms=e0.elapsed_time(e1) / a.block, **{k: round(v, 4) for k, v in phases.items()})
            results["on" if on else "off"].append(rec)
            print(f"[environment cost] round {rnd} {'on ' if on else 'off'}: {json.dumps(rec)}", flush=True)
    summary, ranges = {}, {}
    for key, recs in results.items():
        if recs:
            summary[key] = {k: round(sorted(r[k] for r in recs)[len(recs) // 2], 4) for k in recs[0]}
            ranges[key] = [round(min(r["step_ms"] for r in recs), 4), round(max(r["step_ms"] for r in recs), 4)]
    print(json.dumps(dict(workload=a.workload, n=model.num_gaussians, resolution=a.resolution, overlap=bool(st.overlap_optimizer),
                          block=a.block, rounds=a.rounds, median=summary, step_ms_range=ranges,
                          texels_touched=int((env.texels != 0.5).any(-1).sum()))), flush=True)


if __name__ == "__main__":
    main()
