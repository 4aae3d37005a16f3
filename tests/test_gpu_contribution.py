"""gut_trace_contribution on the device: the per-Gaussian sum and maximum of blending weights and the composited-pixel
count of a view, against the CPU oracle (tests/contribution_reference.py: the cases and their preconditions are asserted by
tests/test_cpu_contribution.py) and against the device's own forward; bit reproducibility; that it disturbs nothing; its refusals;
and, end to end, ContributionScores / keep_mask / compact on a scene with planted invisible rows and in the trainer.

Per case, one view into a zeroed buffer:
  weight_sum  common.check_gradient_rows against the oracle backward's d(sum of red)/d(red feature) with its flip budget and fp32
              conditioning, at that helper's own constants: the bar of every gradient row of this project
  pixels      |gpu - reference| <= the Gaussian's number of flip-prone entries: exact wherever it has none
  max_weight  within COLOUR_TOL of the reference maximum; with prone entries, of the interval between the maxima without and with them
  unwalked    rows without a tile or behind every walked prefix are 16 zero bytes
  forward     sum pixels == sum of the device's hit counts EXACTLY; |sum weight_sum - sum alpha| <= COLOUR_TOL x pixels with a hit"""
import ctypes as C
import importlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests.common import COLOUR_TOL, ROW_FLIP_BOUND, check_gradient_rows, check_gradients_per_row, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
contribution = importlib.import_module("3dgrut_amd.contribution")
_capi = importlib.import_module("3dgrut_amd._capi")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"
PAD = 0xFFFFFFFF


def _device_view(view):
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def _raster(conf=None):
    return gut.Tracer({"render": dict(conf or {})}).tracer_wrapper


def _zeroed(n):
    return torch.zeros((n, 2), dtype=torch.int64, device=DEV)


def _forward(raster, d12, sph, v):
    return raster.trace(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"])


def _score(raster, d12, v, scores):
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores)
    return scores


def _host(scores):
    ws, mw, px = contribution.unpack_scores(scores)
    return ws.cpu().numpy(), mw.cpu().numpy().astype(np.float64), px.cpu().numpy()


@pytest.mark.parametrize("name", cr.CASES)
def test_scores_of_one_view(name):
    case = cr.case(name)
    ref, k, W, H = case["ref"], case["contrib"], case["W"], case["H"]
    n = case["d12"].shape[0]
    raster = _raster(case["conf"])
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    scores = _score(raster, d12, v, _zeroed(n))
    torch.cuda.synchronize()
    ws, mw, px = _host(scores)
    assert raster.stats()["num_intersections"] == ref["M"]

    # against the device's own forward
    hit_sum, alpha_sum = float(hits.double().sum()), float(rgba[..., 3].double().sum())
    with_hit = int((hits > 0).sum())
    print(f"[contribution {name}] pixels {int(px.sum())} vs the forward's hit counts {hit_sum:.0f}; sum of weight_sum {ws.sum():.6f} vs "
          f"sum alpha {alpha_sum:.6f} (bound {COLOUR_TOL * with_hit:.3e}, {with_hit} pixels with a hit)")
    assert int(px.sum()) == int(hit_sum), f"{name}: the walk decides differently from the forward compositor"
    assert abs(ws.sum() - alpha_sum) <= COLOUR_TOL * with_hit

    # weight_sum: the bar of a gradient row
    check_gradient_rows(ws[:, None], case["feat_grad"][:, None], f"contribution {name}/weight_sum", budget=case["flip_budget"], noise=case["fp32_noise"])

    # pixels
    pdiff = np.abs(px - k["pixels"])
    print(f"[contribution {name}] pixel counts differ on {int((pdiff > 0).sum())} Gaussians (allowed on {int((k['prone_entries'] > 0).sum())})")
    assert (pdiff <= k["prone_entries"]).all(), np.nonzero(pdiff > k["prone_entries"])[0][:10]

    # max_weight
    lo, hi = np.minimum(k["max_weight_calm"], k["max_weight"]), k["max_weight"]
    calm = k["prone_entries"] == 0
    worst = float(np.abs(mw - k["max_weight"])[calm].max())
    print(f"[contribution {name}] max_weight: worst difference without a prone entry {worst:.3e}")
    assert worst <= COLOUR_TOL
    assert ((mw >= lo - COLOUR_TOL) & (mw <= hi + COLOUR_TOL)).all()

    # rows the forward did not walk keep their 16 zero bytes
    ordered = raster.debug_buffer("ordered_ids").cpu().numpy().view(np.uint32)
    trav = raster.debug_buffer("tile_traversed_fwd").cpu().numpy().view(np.uint32)
    walked = np.zeros(n, bool)
    for t, (b, e) in enumerate(ref["tile_ranges"]):
        ids = ordered[b:b + min(int(trav[t]), int(e) - int(b))]
        walked[ids[ids != PAD]] = True
    unwalked = ~walked | (ref["tiles_count"] == 0)
    raw = scores.cpu().numpy()
    assert not raw[unwalked].any(), f"{name}: {int(raw[unwalked].any(axis=1).sum())} unwalked rows were written"
    assert not (px[~k["walked"]] != 0).any()
    print(f"[contribution {name}] {int(unwalked.sum())} of {n} rows unwalked and untouched, {int((px > 0).sum())} scored")


def test_identical_inputs_give_identical_bits():
    a, b = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n = 300
    raster = _raster()
    d12, sph = torch.as_tensor(a["d12"], device=DEV), torch.as_tensor(a["sph"], device=DEV)   # one model, the two cases' views
    va, vb = _device_view(a["view"]), _device_view(b["view"])

    _forward(raster, d12, sph, va)
    s1, s2 = _score(raster, d12, va, _zeroed(n)), _score(raster, d12, va, _zeroed(n))   # two calls after one forward
    assert torch.equal(s1, s2) and bool(s1.any())
    _forward(raster, d12, sph, vb)
    sb = _score(raster, d12, vb, _zeroed(n))
    ab = _score(raster, d12, vb, s1.clone())                                                # A then B
    _forward(raster, d12, sph, va)
    ba = _score(raster, d12, va, sb.clone())                                                # B then A
    torch.cuda.synchronize()
    assert torch.equal(ab, ba)
    wa, wb = s1.view(torch.int32).reshape(-1, 4), sb.view(torch.int32).reshape(-1, 4)
    combined = torch.stack([s1[:, 0] + sb[:, 0],
                            (torch.maximum(wa[:, 2], wb[:, 2]).to(torch.int64) & 0xFFFFFFFF) | ((wa[:, 3].to(torch.int64) + wb[:, 3].to(torch.int64)) << 32)], 1)
    assert torch.equal(ab, combined)    # integer sum, max of the (non-negative) float bits, integer sum


def test_nothing_else_changes():
    case = cr.case("pinhole_64x48")
    n, W, H = 300, case["W"], case["H"]
    raster = _raster()
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    # (a first forward and backward, so that the handle has gradient rows to show: every consumer leaves them zero)
    outs = _forward(raster, d12, sph, v)
    raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.ones_like(outs[0]), outs[1], None)
    outs = _forward(raster, d12, sph, v)
    before = [o.clone() for o in outs]
    _score(raster, d12, v, _zeroed(n))
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b)
    assert not bool(raster.debug_buffer("grad_scratch").any())
    # a backward follows as if nothing had happened
    rgba_grad = np.random.default_rng(11).normal(size=(H, W, 4)).astype(np.float32)
    g12, g48 = raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.as_tensor(rgba_grad, device=DEV), outs[1], None)
    dens_g, sph_g, _, budget = oracle.backward(case["view"]["oracle_cam"], case["ref"], rgba_grad, np.zeros((H, W, 1), np.float32),
                                               flip_bound=ROW_FLIP_BOUND)
    check_gradients_per_row(g12.cpu().numpy(), g48.cpu().numpy(), dens_g, sph_g, "backward after trace_contribution", budget=budget)


def _raw_call(raster, n, d12, v, scores_ptr, stream=None, W=None, H=None):
    cam = raster._camera(*v["tail"])
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    H0, W0 = int(v["ro"].shape[1]), int(v["ro"].shape[2])
    return raster._lib.gut_trace_contribution(raster._handle, C.c_void_p(st), 0, 3, n, d12.data_ptr(), W or W0, H or H0,
                                              v["ro"].data_ptr(), v["rd"].data_ptr(), C.byref(cam), scores_ptr)


def test_refusals_leave_the_handle_rendering():
    case, other = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n = 300
    v, vo = _device_view(case["view"]), _device_view(other["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    raster = _raster()
    sentinel = _zeroed(n)

    def refused(pattern, call):
        with pytest.raises(RuntimeError, match=pattern):
            call()
        torch.cuda.synchronize()
        assert not bool(sentinel.any()), f"{pattern!r}: the refused call wrote scores"

    def raw(*a, **kw):
        _capi.check(_raw_call(raster, *a, **kw), "trace_contribution")

    refused(re.escape("gut_trace_contribution: no forward context on this stream"), lambda: _score(raster, d12, v, sentinel))
    ref_out = [o.clone() for o in _forward(raster, d12, sph, v)]
    side = torch.cuda.Stream(DEV)
    refused(re.escape("gut_trace_contribution: no forward context on this stream"),
            lambda: raw(n, d12, v, sentinel.data_ptr(), stream=side.cuda_stream))
    refused(re.escape(f"gut_trace_contribution: arguments differ from the cached forward (N {n - 1} vs {n}"),
            lambda: _score(raster, d12[:n - 1], v, sentinel[:n - 1]))
    refused(re.escape("gut_trace_contribution: camera differs from the cached forward"),
            lambda: raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *vo["tail"], sentinel))
    refused(re.escape("gut_trace_contribution: d_scores is NULL"), lambda: raw(n, d12, v, None))
    refused(re.escape("gut_trace_contribution: d_scores must be 8-byte aligned"), lambda: raw(n, d12, v, sentinel.data_ptr() + 4))
    # the handle still scores and renders as an untouched one
    got = _score(raster, d12, v, _zeroed(n))
    fresh = _raster()
    _forward(fresh, d12, sph, v)
    want = _score(fresh, d12, v, _zeroed(n))
    again = _forward(raster, d12, sph, v)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(got.any())
    for o, b in zip(again, ref_out):
        assert torch.equal(o, b)

    for conf, what in (({"splat": {"k_buffer_size": 16}}, "k_buffer_size=16"), ({"particle_kernel_degree": 4}, "particle_kernel_degree=4")):
        r = _raster(conf)
        out = [o.clone() for o in _forward(r, d12, sph, v)]
        with pytest.raises(RuntimeError, match=re.escape("supported on the unsorted variant (k_buffer_size=0) at particle_kernel_degree=2 only") + ".*" + re.escape(what)):
            _score(r, d12, v, sentinel)
        torch.cuda.synchronize()
        assert not bool(sentinel.any())
        for o, b in zip(_forward(r, d12, sph, v), out):
            assert torch.equal(o, b)


def _device_view_of_batch(scorer, batch):
    sensor, poses = scorer._create_camera(batch)
    return (batch.rays_ori.contiguous(), batch.rays_dir.contiguous(),
            (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def test_rows_no_view_sees_score_nothing_and_compaction_keeps_the_renders():
    """densified_like_scene(20000) plus 2000 planted rows no view can see (contribution_reference.planted_scene: the oracle gives
    them no weight in any of the six views), six orbit views at 160 x 120.  Every planted row scores pixels == 0; dropping every row
    with pixels == 0 removes at least those; and the six renders of the compacted model stay within COLOUR_TOL per pixel of the
    original ones: a kernel that loses a contribution removes a row that is seen, and fails here."""
    native = importlib.import_module("3dgrut_amd.native")
    sc, planted = cr.planted_scene()
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    batches = [to_batch(v, DEV) for v in cr.planted_views()]
    stepper = native.NativeTrainStep(model, tracer, scene_extent=1.0)
    with torch.no_grad():
        before = [tracer.render(model, b, train=False) for b in batches]
        before = [torch.cat([o["pred_rgb"][0], o["pred_opacity"][0]], -1).clone() for o in before]
    scorer = contribution.ContributionScores(model, tracer)
    hits = 0
    for b in batches:
        scorer.accumulate(b)
        # the hit counts of the forward the scores belong to: the same packed rows once more (Tracer.render activates the model's
        # rows by another route, whose last bits — and with them a decision in a million — may differ)
        v = _device_view_of_batch(scorer, b)
        hits += int(scorer.raster.trace(0, scorer.n_active_features, scorer.act, scorer.features, v[0], v[1], None, *v[2])[2].double().sum())
    res = scorer.result()
    assert res["n_views"] == 6 and res["weight_sum"].dtype == torch.float64 and res["max_weight"].dtype == torch.float32 and res["pixels"].dtype == torch.int64
    px = res["pixels"].cpu().numpy()
    assert not px[planted].any(), f"{int((px[planted] > 0).sum())} planted rows were scored"
    assert ((res["weight_sum"] > 0) == (res["pixels"] > 0)).all() and ((res["max_weight"] > 0) == (res["pixels"] > 0)).all()
    assert int(res["pixels"].sum()) == hits     # exactly the composited (view, pixel, Gaussian) triples of the six forwards
    alpha = sum(float(b[..., 3].double().sum()) for b in before)
    assert abs(float(res["weight_sum"].sum()) - alpha) <= COLOUR_TOL * 6 * 160 * 120
    mask = contribution.keep_mask(res, min_pixels=1)
    n = model.num_gaussians
    removed = contribution.compact(stepper, mask)
    kept = n - removed
    print(f"[compaction] {n} rows, {int((px > 0).sum())} scored, {removed} removed (2000 planted), {kept} kept")
    assert removed >= 2000 and model.num_gaussians == kept == int((px > 0).sum())
    assert stepper.m12.shape[0] == kept and stepper.v48.shape[0] == kept
    with torch.no_grad():
        for i, b in enumerate(batches):
            o = tracer.render(model, b, train=False)
            diff = float((torch.cat([o["pred_rgb"][0], o["pred_opacity"][0]], -1) - before[i]).abs().max())
            print(f"[compaction] view {i}: the compacted model's render differs by {diff:.3e}")
            assert diff <= COLOUR_TOL


@pytest.fixture(scope="module")
def colmap_dir(tmp_path_factory):
    from tests.synthetic_colmap import write_synthetic_colmap
    return write_synthetic_colmap(str(tmp_path_factory.mktemp("synthetic_colmap_contribution")))


TRAINER_ARGS = ["--n-iterations", "200", "--compact-to", "0.5", "--compact-finetune", "20"]


def test_trainer_cli_compacts_and_its_checkpoint_resumes(colmap_dir, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "3dgrut_amd.trainer", "--path", colmap_dir, "--out-dir", str(tmp_path)] + TRAINER_ARGS,
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    s = last["stats"]
    print(f"[trainer cli] {s}\n[trainer cli] test {last['test']}")
    assert {"compaction_n_before", "compaction_n_after", "compaction_score", "compaction_test_psnr_before"} <= set(s)
    assert s["compaction_n_after"] == math.ceil(0.5 * s["compaction_n_before"]) and s["compaction_score"] == "weight_sum"
    assert s["n_steps"] == 220 and s["n_gaussians"] == s["compaction_n_after"]
    assert s["compaction_test_psnr_before"] > 0 and last["test"]["mean_psnr"] > 0
    path = os.path.join(str(tmp_path), "ckpt_last.pt")
    ckpt = torch.load(path, weights_only=True)
    n = s["compaction_n_after"]
    assert ckpt["positions"].shape[0] == n and ckpt["features_specular"].shape[0] == n and ckpt["global_step"] == 220
    for st in ckpt["optimizer"]["state"].values():
        assert st["exp_avg"].shape[0] == n and st["exp_avg_sq"].shape[0] == n
    from tests.synthetic_colmap import load_scene
    trainer_mod = importlib.import_module("3dgrut_amd.trainer")
    _, tb, vb, extent = load_scene(colmap_dir)
    resumed = trainer_mod.Trainer(dict(n_iterations=225, resume=path, out_dir="", test_last=False, val_frequency=10 ** 9), None, tb,
                                  test_batches=vb, scene_extent=extent)
    assert resumed.model.num_gaussians == n and resumed.global_step == 220
    resumed.train()
    assert resumed.global_step == 225 and bool(torch.isfinite(resumed.model.raw).all())


def test_scores_choose_better_than_chance(colmap_dir):
    """Two runs of the same code on the same data that differ in one thing: which half of the rows leaves at the compaction point —
    the worst by contribution, or as many rows chosen uniformly at random (seeded).  The final held-out PSNR of the first is not
    below the second's.  A run without the block has none of the new statistics."""
    from tests.synthetic_colmap import load_scene
    trainer_mod = importlib.import_module("3dgrut_amd.trainer")
    init, tb, vb, extent = load_scene(colmap_dir)
    ap = trainer_mod.build_parser()

    def run(args, random_rows):
        conf = trainer_mod.config_from_args(ap.parse_args(["--path", colmap_dir] + args))
        conf["out_dir"] = ""
        tr = trainer_mod.Trainer(conf, init, tb, val_batches=vb, test_batches=vb, scene_extent=extent)
        if random_rows:
            by_score = tr._compaction_mask

            def at_random(result):
                keep = int(by_score(result).sum())
                n = int(result["pixels"].shape[0])
                idx = torch.randperm(n, generator=torch.Generator().manual_seed(7))[:keep]
                mask = torch.zeros(n, dtype=torch.bool)
                mask[idx] = True
                return mask.to(result["pixels"].device)
            tr._compaction_mask = at_random
        return tr.run()

    scored, chance, plain = run(TRAINER_ARGS, False), run(TRAINER_ARGS, True), run(["--n-iterations", "200"], False)
    a, b = scored["test"]["mean_psnr"], chance["test"]["mean_psnr"]
    print(f"[trainer] N {scored['stats']['compaction_n_before']} -> {scored['stats']['compaction_n_after']}: test psnr before "
          f"{scored['stats']['compaction_test_psnr_before']:.3f}, after by score {a:.3f}, after at random {b:.3f}; uncompacted run {plain['test']['mean_psnr']:.3f}")
    assert scored["stats"]["compaction_n_after"] == chance["stats"]["compaction_n_after"] == math.ceil(0.5 * scored["stats"]["compaction_n_before"])
    assert a >= b
    assert not any(k.startswith("compaction") for k in plain["stats"])
    assert set(plain["stats"]) == {"n_steps", "n_epochs", "steps_run", "training_time", "iteration_speed", "n_gaussians"}
