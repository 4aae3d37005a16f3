"""Dev probe (GPU): what the forms of the contribution walk (DESIGN.md §13–§15, §17, §18) cost on a bench workload, next to the forward
compositor they re-walk.

Per iteration: a forward of one of eight orbit views on frozen, packed rows (FrozenModel's), then every requested form, each timed
event to event (the tile order plus the form's launches); the forward compositor's time of the SAME forward comes from the library's
kernel timers (gut_kernel_times: `render`).  Prints one JSON line: the medians over the timed iterations and their ratios.

    plain           gut_trace_contribution; also the walked list entries of the last forward (an upper bound of the records the flush
                    updates) and how many rows ended up scored
    weighted        after the plain walk (timed with it), the walk that writes both records with a per-pixel plane
                    (gut_trace_contribution_weighted) and the error plane itself (gut_pixel_error against a stand-in photo)
    attributes      gut_trace_attributes at every K of --channels (one walk per group of four channels)
    attributes_bwd  gut_trace_attributes_bwd at every K of --channels (per group two memsets, the planes' maxima, the walk and the
                    pass over the rows)
    surface         gut_trace_surface in both modes (level 0.5 and the largest weight), all three planes written

    python tools/walk_cost.py [--forms plain,weighted,attributes,attributes_bwd,surface] [--channels 1,4,8]
                              [--workload bicycle_like_6M_1237x822] [--num-gaussians N] [--iterations 48] [--warmup 8]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("plain", "weighted", "attributes", "attributes_bwd", "surface")


def spread(key, ms):
    return {f"{key}_ms_median": statistics.median(ms), f"{key}_ms_min": min(ms), f"{key}_ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--channels", default="1,4,8")
    ap.add_argument("--workload", default="bicycle_like_6M_1237x822")
    ap.add_argument("--num-gaussians", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    forms = a.forms.split(",")
    if not forms or any(f not in FORMS for f in forms):
        ap.error("--forms: a comma-separated list of " + ", ".join(FORMS))
    channels = tuple(int(k) for k in a.channels.split(","))
    import torch
    bench = importlib.import_module("bench")
    gut = importlib.import_module("3dgrut_amd")
    native = importlib.import_module("3dgrut_amd.native")
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    contribution = importlib.import_module("3dgrut_amd.contribution")
    losses = importlib.import_module("3dgrut_amd.losses")
    if not torch.cuda.is_available():
        raise SystemExit("walk_cost: no GPU (there is nothing to time on a CPU)")
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
    raster, act, n = scorer.raster, scorer.act, int(scorer.act.shape[0])
    gen = torch.Generator(device=dev).manual_seed(0)
    # (the kernels' times do not depend on the values)
    both = torch.zeros_like(scorer.scores)
    weighted = torch.zeros((n,), dtype=torch.int64, device=dev)
    photo = torch.rand((H, W, 3), generator=gen, device=dev)   # a stand-in
    plane = torch.empty((H, W), dtype=torch.float32, device=dev)
    rows = {k: torch.rand((n, k), generator=gen, device=dev) for k in channels}
    planes = {k: torch.empty((k, H, W), dtype=torch.float32, device=dev) for k in channels}
    cots = {k: torch.rand((k, H, W), generator=gen, device=dev) * 2.0 - 1.0 for k in channels}
    grads = {k: torch.empty((n, k), dtype=torch.float32, device=dev) for k in channels}
    surf = (torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev),
            torch.empty((H, W), dtype=torch.float32, device=dev))
    times = {}   # key -> the timed iterations' milliseconds

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
        rgba = raster.trace(0, 3, act, scorer.features, ro_t, rd_t, None, *cam)[0]
        events = {}
        if "plain" in forms or "weighted" in forms:
            events["contribution"] = timed(lambda: raster.trace_contribution(0, 3, act, ro_t, rd_t, *cam, scorer.scores))
        if "weighted" in forms:
            events["pixel_error"] = timed(lambda: losses.fused_pixel_error(rgba, photo, 0.0, out=plane))
            events["weighted"] = timed(lambda: raster.trace_contribution(0, 3, act, ro_t, rd_t, *cam, both, pixel_weight=plane, weighted=weighted))
        for k in channels:
            if "attributes" in forms:
                events[f"attributes_k{k}"] = timed(lambda: raster.trace_attributes(0, 3, act, rows[k], ro_t, rd_t, *cam, out=planes[k]))
            if "attributes_bwd" in forms:
                events[f"attributes_bwd_k{k}"] = timed(lambda: raster.trace_attributes_bwd(0, 3, act, cots[k], ro_t, rd_t, *cam, out=grads[k]))
        if "surface" in forms:
            for mode in ("level", "max_weight"):
                events[f"surface_{mode}"] = timed(lambda: raster.trace_surface(0, 3, act, ro_t, rd_t, *cam, mode=mode, level=0.5,
                                                                               with_id=True, with_weight=True, out=surf))
        torch.cuda.synchronize(dev)
        if it >= a.warmup:
            times.setdefault("render", []).append(raster.kernel_times()["render"])
            for key, (e0, e1) in events.items():
                times.setdefault(key, []).append(e0.elapsed_time(e1))
    st = raster.stats()
    render = statistics.median(times["render"])
    out = dict(workload=a.workload, n=n, iterations=a.iterations, **spread("render", times["render"]),
               traversed_fwd_last_view=st["traversed_fwd"], intersections_last_view=st["num_intersections"])
    if "contribution" in times:
        res = scorer.result()
        out.update(**spread("contribution", times["contribution"]), ratio_of_medians=statistics.median(times["contribution"]) / render,
                   rows_scored=int((res["pixels"] > 0).sum()), pixels_total=int(res["pixels"].sum()))
    if "weighted" in times:
        assert torch.equal(both, scorer.scores)      # the records of the walk that writes both are the plain walk's
        out.update(**spread("weighted", times["weighted"]), **spread("pixel_error", times["pixel_error"]),
                   weighted_over_plain=statistics.median(times["weighted"]) / statistics.median(times["contribution"]),
                   weighted_over_render=statistics.median(times["weighted"]) / render, rows_with_error=int((weighted > 0).sum()))
    for key in times:
        if key.startswith(("attributes", "surface")):
            out.update(**spread(key, times[key]), **{f"{key}_over_render": statistics.median(times[key]) / render})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
