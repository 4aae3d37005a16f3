"""Dev probe (GPU): the native train step with the MCMC regularisers off and on (strategy.MCMC_LOSS), alternating in one process on
the bench stand-ins, in steady state (after the overlap probe and the placement tuning).  Prints ms per step (event-timed per step:
median and spread) for each setting and round, and one JSON line at the end.

    python tools/regulariser_cost.py [--workloads bicycle_like_6M_1237x822,bicycle_like_6M_surface] [--rounds 3] [--steps 20]
"""
import argparse
import gc
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

gut = importlib.import_module("3dgrut_amd")
scenes = importlib.import_module("3dgrut_amd.scenes")
cams = importlib.import_module("3dgrut_amd.cameras")
native = importlib.import_module("3dgrut_amd.native")
strategy = importlib.import_module("3dgrut_amd.strategy")


def run(workload, rounds, steps):
    dev = torch.device("cuda", 0)
    fn, kw, W, H, fx, radius, elev, extent = bench.WORKLOADS[workload]
    model = native.NativeGaussianModel(getattr(scenes, fn)(**kw), device=dev, spatial_order=True)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=extent)
    bench.synthetic_optimizer_state(st)
    ro, rd, c2ws = bench.make_views(cams, 8, W, H, fx, radius, elev)
    ro_t, rd_t = torch.as_tensor(ro, device=dev), torch.as_tensor(rd, device=dev)
    K = cams.pinhole_intrinsics_dict(W, H, fx, fx)
    gt = torch.rand((1, H, W, 3), device=dev)

    def batch(i):
        return gut.Batch(rays_ori=ro_t, rays_dir=rd_t, T_to_world=torch.as_tensor(c2ws[i % 8])[None], rgb_gt=gt,
                         intrinsics_OpenCVPinholeCameraModelParameters=K)

    for i in range(2):
        st.step(batch(i))
    st.tune_placement()
    for i in range(12):                      # past the overlap probe (steps 2..9)
        st.step(batch(i))
    res = {"off": [], "on": []}
    for r in range(rounds):
        for name, lam in (("off", 0.0), ("on", strategy.MCMC_LOSS)):
            st.lambda_opacity = 0.0 if lam == 0.0 else lam["lambda_opacity"]
            st.lambda_scale = 0.0 if lam == 0.0 else lam["lambda_scale"]
            for i in range(4):               # the switch's sync and a few steps in the new setting
                st.step(batch(i))
            torch.cuda.synchronize()
            gc.collect()
            ms = []
            for i in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st.step(batch(i))
                e1.record()
                ms.append((e0, e1))
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(b) for a, b in ms)
            res[name] += t
            print(f"{workload} round {r} regulariser {name}: median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}", flush=True)
    out = {"workload": workload, "overlap_optimizer": bool(st.overlap_optimizer)}
    for name, t in res.items():
        t = sorted(t)
        out[name] = dict(median_ms=round(t[len(t) // 2], 4), p10_ms=round(t[len(t) // 10], 4), p90_ms=round(t[(9 * len(t)) // 10], 4))
    out["ratio_on_off"] = round(out["on"]["median_ms"] / out["off"]["median_ms"], 4)
    del st, model
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bicycle_like_6M_1237x822,bicycle_like_6M_surface")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    results = [run(w, a.rounds, a.steps) for w in a.workloads.split(",")]
    print(json.dumps(results))


if __name__ == "__main__":
    main()
