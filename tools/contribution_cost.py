"""Dev probe (GPU): what gut_trace_contribution costs on a bench workload, next to the forward compositor it re-walks.

Per iteration: a forward of one of eight orbit views on frozen, packed rows (ContributionScores' own), then the contribution walk timed
event to event (its two launches: the tile order and k_contribution); the forward compositor's time of the SAME forward comes from
the library's kernel timers (gut_kernel_times: `render`).  Prints the medians over the timed iterations, the walked list entries of
the last forward (an upper bound of the records the flush updates) and how many rows ended up scored.

--weighted: on the same forwards, after the plain walk, also the walk that writes both records with a per-pixel plane
(gut_trace_contribution_weighted) and the error plane itself (gut_pixel_error against a stand-in photo), each timed event to event.

    python tools/contribution_cost.py [--workload bicycle_like_6M_1237x822] [--iterations 48] [--warmup 8] [--weighted]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle_like_6M_1237x822")
    ap.add_argument("--num-gaussians", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--weighted", action="store_true", help="also time the weighted walk and gut_pixel_error on the same forwards")
    a = ap.parse_args()
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    contribution = importlib.import_module("3dgrut_amd.contribution")
    losses = importlib.import_module("3dgrut_amd.losses")
    if not torch.cuda.is_available():
        raise SystemExit("contribution_cost: no GPU (there is nothing to time on a CPU)")
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
    scorer = contribution.ContributionScores(model, tracer)
    raster = scorer.raster
    walk_ms, render_ms, both_ms, error_ms = [], [], [], []
    if a.weighted:
        both = torch.zeros_like(scorer.scores)
        weighted = torch.zeros((scorer.act.shape[0],), dtype=torch.int64, device=dev)
        photo = torch.rand((H, W, 3), generator=torch.Generator(device=dev).manual_seed(0), device=dev)   # a stand-in: the kernel's time does not depend on it
        plane = torch.empty((H, W), dtype=torch.float32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1
    for it in range(a.warmup + a.iterations):
        batch = batches[it % n_views]
        sensor, poses = scorer._create_camera(batch)
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        rgba = raster.trace(0, 3, scorer.act, scorer.features, ro_t, rd_t, None, *cam)[0]
        e0, e1 = timed(lambda: raster.trace_contribution(0, 3, scorer.act, ro_t, rd_t, *cam, scorer.scores))
        if a.weighted:
            p0, p1 = timed(lambda: losses.fused_pixel_error(rgba, photo, 0.0, out=plane))
            w0, w1 = timed(lambda: raster.trace_contribution(0, 3, scorer.act, ro_t, rd_t, *cam, both, pixel_weight=plane, weighted=weighted))
        torch.cuda.synchronize(dev)
        if it >= a.warmup:
            walk_ms.append(e0.elapsed_time(e1))
            render_ms.append(raster.kernel_times()["render"])
            if a.weighted:
                error_ms.append(p0.elapsed_time(p1))
                both_ms.append(w0.elapsed_time(w1))
    st = raster.stats()
    res = scorer.result()
    out = dict(workload=a.workload, n=int(model.num_gaussians), iterations=a.iterations,
               contribution_ms_median=statistics.median(walk_ms), contribution_ms_min=min(walk_ms), contribution_ms_max=max(walk_ms),
               render_ms_median=statistics.median(render_ms), render_ms_min=min(render_ms), render_ms_max=max(render_ms),
               ratio_of_medians=statistics.median(walk_ms) / statistics.median(render_ms),
               traversed_fwd_last_view=st["traversed_fwd"], intersections_last_view=st["num_intersections"],
               rows_scored=int((res["pixels"] > 0).sum()), pixels_total=int(res["pixels"].sum()))
    if a.weighted:
        assert torch.equal(both, scorer.scores)      # the records of the walk that writes both are the plain walk's
        out.update(weighted_ms_median=statistics.median(both_ms), weighted_ms_min=min(both_ms), weighted_ms_max=max(both_ms),
                   pixel_error_ms_median=statistics.median(error_ms), pixel_error_ms_min=min(error_ms), pixel_error_ms_max=max(error_ms),
                   weighted_over_plain=statistics.median(both_ms) / statistics.median(walk_ms),
                   rows_with_error=int((weighted > 0).sum()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
