"""Dev probe (GPU): what gut_trace_attributes_bwd costs on a bench workload, next to the forward compositor it
re-walks and to gut_trace_attributes, its other direction.

Per iteration: a forward of one of eight orbit views on frozen, packed rows (AttributeRenderer's own), then the attribute walk and
its backward at K = 1, 4 and 8 channels, each timed event to event (the backward: the tile order and, per group of four channels,
two memsets, the planes' maxima, the walk and the pass over the rows); the forward compositor's time of the SAME forward comes from
the library's kernel timers (gut_kernel_times: `render`).  Prints the medians over the timed iterations and their ratios to the
compositor's.

    python tools/attribute_gradient_cost.py [--workload bicycle_like_6M_1237x822] [--iterations 48] [--warmup 8]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS = (1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle_like_6M_1237x822")
    ap.add_argument("--num-gaussians", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    attributes = importlib.import_module("3dgrut_amd.attributes")
    if not torch.cuda.is_available():
        raise SystemExit("attribute_gradient_cost: no GPU (there is nothing to time on a CPU)")
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[a.workload]
    kw = dict(kw)
    if a.num_gaussians:
        kw["n"] = a.num_gaussians
    scene = getattr(scenes, fn)(**kw)
    tracer = gut.Tracer({"render": {"enable_kernel_timings": True}})
    model = native.NativeGaussianModel(scene, device=dev, sh_degree=3, spatial_order=True)
    n_views = 8
    ro, rd, c2ws = bench.make_views(cams, n_views, W, H, fx, radius, elev, False)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    batches = [gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[v])[None],
                         intrinsics_OpenCVPinholeCameraModelParameters=K) for v in range(n_views)]
    renderer = attributes.AttributeRenderer(model, tracer)
    raster, n = renderer.raster, int(renderer.act.shape[0])
    gen = torch.Generator(device=dev).manual_seed(0)
    # (the kernels' times do not depend on the values)
    rows = {k: torch.rand((n, k), generator=gen, device=dev) for k in CHANNELS}
    planes = {k: torch.empty((k, H, W), dtype=torch.float32, device=dev) for k in CHANNELS}
    cots = {k: torch.rand((k, H, W), generator=gen, device=dev) * 2.0 - 1.0 for k in CHANNELS}
    grads = {k: torch.empty((n, k), dtype=torch.float32, device=dev) for k in CHANNELS}
    fwd_ms, bwd_ms, render_ms = {k: [] for k in CHANNELS}, {k: [] for k in CHANNELS}, []

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1
    for it in range(a.warmup + a.iterations):
        batch = batches[it % n_views]
        sensor, poses = renderer._create_camera(batch)
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        raster.trace(0, 3, renderer.act, renderer.features, ro_t, rd_t, None, *cam)
        fwd = {k: timed(lambda k=k: raster.trace_attributes(0, 3, renderer.act, rows[k], ro_t, rd_t, *cam, out=planes[k])) for k in CHANNELS}
        bwd = {k: timed(lambda k=k: raster.trace_attributes_bwd(0, 3, renderer.act, cots[k], ro_t, rd_t, *cam, out=grads[k])) for k in CHANNELS}
        torch.cuda.synchronize(dev)
        if it >= a.warmup:
            render_ms.append(raster.kernel_times()["render"])
            for k in CHANNELS:
                fwd_ms[k].append(fwd[k][0].elapsed_time(fwd[k][1]))
                bwd_ms[k].append(bwd[k][0].elapsed_time(bwd[k][1]))
    st = raster.stats()
    render = statistics.median(render_ms)
    out = dict(workload=a.workload, n=n, iterations=a.iterations, render_ms_median=render, render_ms_min=min(render_ms),
               render_ms_max=max(render_ms), traversed_fwd_last_view=st["traversed_fwd"], intersections_last_view=st["num_intersections"])
    for what, ms in (("attributes", fwd_ms), ("attributes_bwd", bwd_ms)):
        for k in CHANNELS:
            med = statistics.median(ms[k])
            out.update({f"{what}_k{k}_ms_median": med, f"{what}_k{k}_ms_min": min(ms[k]), f"{what}_k{k}_ms_max": max(ms[k]),
                        f"{what}_k{k}_over_render": med / render})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
