"""Dev probe (GPU): what per-view bilateral grids (gut_bilateral_slice before the loss, gut_bilateral_backward and the
view's Adam step behind it) cost.  Two measurements in one run, on one box:

  kernels   the slice alone, and the four-launch adjoint (maximum, scatter, conversion with the TV term, Adam step) alone, on a
            random image of the workload's resolution, event to event over `--calls` calls;
  step      one NativeTrainStep(bilateral_gradient=True) on the workload's scene, built as bench.py builds it; blocks of `--block`
            steps alternate between batches without a grid (the parent's launch list) and with one, `--rounds` times, each block
            timed event to event and by phase (phase_times_mean).

    python tools/bilateral_cost.py [--workload bicycle_like_6M_1237x822] [--grid 16 16 8] [--block 24] [--rounds 4] [--warmup 16]
    python tools/bilateral_cost.py --kernels-only
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bilateral_cost.py --kernels-only      # the five kernels' own times
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_kernels(torch, bilateral, dev, H, W, triple, calls, lambda_tv):
    """Median-free and simple: `calls` back-to-back calls between two events, after as many untimed ones."""
    grids = bilateral.BilateralGrids(1, triple, dev, lambda_tv=lambda_tv)
    gen = torch.Generator().manual_seed(7)
    rgba = torch.rand((H, W, 4), generator=gen).to(dev)
    out_grad = (torch.randn((H, W, 4), generator=gen) / (H * W)).to(dev)
    grids.params[0].add_(0.05 * torch.randn(grids.params[0].shape, generator=gen).to(dev))
    out, image, grad = torch.empty_like(rgba), torch.empty_like(rgba), torch.empty_like(grids.params[0])

    def timed(fn):
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def adjoint():
        grids.backward(0, rgba, 0.0, out_grad, rgba_grad=image, grid_grad=grad)
        grids.end(0, grad)
    return dict(slice_ms=round(timed(lambda: grids.slice(0, rgba, 0.0, out=out)), 4), adjoint_ms=round(timed(adjoint), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle_like_6M_1237x822")
    ap.add_argument("--num-gaussians", type=int, default=0)
    ap.add_argument("--grid", type=int, nargs=3, default=[16, 16, 8], metavar=("X", "Y", "L"))
    ap.add_argument("--lambda-tv", type=float, default=10.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--block", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--kernels-only", action="store_true", help="skip the train step (profiler runs)")
    a = ap.parse_args()
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    bilateral = importlib.import_module("3dgrut_amd.bilateral")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    if not torch.cuda.is_available():
        raise SystemExit("bilateral_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[a.workload]
    kernels = time_kernels(torch, bilateral, dev, H, W, tuple(a.grid), a.calls, a.lambda_tv)
    print(f"[bilateral cost] kernels alone at {W}x{H}, grid {a.grid}: {json.dumps(kernels)}", flush=True)
    if a.kernels_only:
        print(json.dumps(dict(workload=a.workload, grid=a.grid, kernels=kernels)), flush=True)
        return
    kw = dict(kw)
    if a.num_gaussians:
        kw["n"] = a.num_gaussians
    scene = getattr(scenes, fn)(**kw)
    tracer = gut.Tracer({"render": {}})
    model = native.NativeGaussianModel(scene, device=dev, sh_degree=3, spatial_order=True)
    st = native.NativeTrainStep(model, tracer, scene_extent=extent, bilateral_gradient=True)
    bench.synthetic_optimizer_state(st)
    n_views = 8
    grids = bilateral.BilateralGrids(n_views, tuple(a.grid), dev, lambda_tv=a.lambda_tv)
    ro, rd, c2ws = bench.make_views(cams, n_views, W, H, fx, radius, elev, False)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(100)).to(dev)
    batches = [gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[v])[None], rgb_gt=gt,
                         intrinsics_OpenCVPinholeCameraModelParameters=K) for v in range(n_views)]

    step = 0

    def one(on):
        nonlocal step
        v = step % n_views
        st.step(grids.begin(v, batches[v]) if on else batches[v])
        if on:
            grids.end(v, st.bilateral_gradient)
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
            rec = dict(step_ms=e0.elapsed_time(e1) / a.block, **{k: round(v, 4) for k, v in phases.items()})
            results["on" if on else "off"].append(rec)
            print(f"[bilateral cost] round {rnd} {'on ' if on else 'off'}: {json.dumps(rec)}", flush=True)
    summary, ranges = {}, {}
    for key, recs in results.items():
        if recs:
            summary[key] = {k: round(sorted(r[k] for r in recs)[len(recs) // 2], 4) for k in recs[0]}
            ranges[key] = [round(min(r["step_ms"] for r in recs), 4), round(max(r["step_ms"] for r in recs), 4)]
    print(json.dumps(dict(workload=a.workload, n=model.num_gaussians, grid=a.grid, overlap=bool(st.overlap_optimizer), block=a.block,
                          rounds=a.rounds, kernels=kernels, median=summary, step_ms_range=ranges)), flush=True)


if __name__ == "__main__":
    main()
