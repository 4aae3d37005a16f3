"""Pose alignment of held-out views on the GPU: the pose-only backward (gut_trace_bwd_pose) against the float64
definition on the dense gradient a plain backward of a second handle returns, what it leaves in the handle, its refusals, and
evaluate(pose_aligned=...) on perturbed, exact and unexplainable views, with colour correction, on a live trainer and from the
command line."""
import copy
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.common import cams, make_view, pose, scenes, to_batch
from tests.synthetic_colmap import write_synthetic_colmap
from tests.test_gpu_pose_gradient import CASES, LOOK_AT, _orbit_batches, _rows, _trace_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
gut = importlib.import_module("3dgrut_amd")
tracer_mod = importlib.import_module("3dgrut_amd.tracer")
native = importlib.import_module("3dgrut_amd.native")
evaluate_mod = importlib.import_module("3dgrut_amd.evaluate")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P_ROT, P_POS = 0.01, 0.02      # the recovery test's perturbation: 0.01 rad and 0.02 in centre position, under two pixels
RECOVERY = dict(iterations=60, lr_translation=P_POS / 20, lr_rotation=P_ROT / 20)


def _pose_args(args):
    """_trace_args' tuple (trace / trace_bwd order) in trace_bwd_pose's order: no radiance rows, no ray_time."""
    return (args[0], args[1], args[2], args[4], args[5], *args[7:12])


def _cotangent(rgba, seed):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal(tuple(rgba.shape)).astype(np.float32), device=DEV)


# ---- 1. the kernel ----
@pytest.mark.parametrize("name", list(CASES))
def test_pose_only_backward_equals_the_definition_and_leaves_the_rows_zero(name):
    """out8 of trace_bwd_pose against pose_gradient_from_rows in float64 on the dense gradient a plain trace_bwd of a SECOND handle
    returns for the same rows and cotangent: |got_k - ref_k| <= 2e-5 S_k, the project's bar for two backwards whose atomics sum in
    different orders (1e-5 S_k for the reduction, as much again for the rows).  The cotangent seed is the first of 0..7 for which
    the reference alone gives |ref_k| >= 1e-3 S_k.  Slot 6 is the number of rows with a tile, slot 7 is 0.  Afterwards the gradient
    scratch is all zeros, and a following forward + plain backward on the same handle returns the dense gradient of the fresh
    handle within rtol 1e-3, atol 1e-4 max (a stale row would double it)."""
    c = CASES[name]
    sc = scenes.scene_c1(c["n"], 0)
    act, sph = _rows(sc)
    n = act.shape[0]
    view = make_view(c["kind"], c["W"], c["H"], cams.look_at_c2w(*LOOK_AT), distortion=c.get("distortion"))
    conf = {"render": {"splat": {"k_buffer_size": c.get("k_buffer", 0)}}}
    raster, other = tracer_mod.SplatRaster(conf), tracer_mod.SplatRaster(conf)
    cam_pos = np.asarray(view["c2w"], np.float64)[:3, 3]
    args = _trace_args(view, act, sph)
    for seed in range(8):
        rgba, dist, _, _ = other.trace(*args)
        cot = _cotangent(rgba, seed)
        dense, _ = other.trace_bwd(*args, rgba, cot, dist, None)
        terms = pose.pose_gradient_terms(act, dense, cam_pos)
        ref, S = terms.sum(0).cpu(), terms.abs().sum(0).cpu()
        if bool((ref.abs() >= 1e-3 * S).all()):
            break
    else:
        pytest.fail(f"{name}: no cotangent seed below 8 gives |ref_k| >= 1e-3 S_k for every k")
    out8 = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    raster.set_pose_gradient(out8)
    rgba, dist, _, _ = raster.trace(*args)
    assert raster.trace_bwd_pose(*_pose_args(args), rgba, cot, dist, None) is None
    got = out8.cpu().double()
    err = (got[:6] - ref).abs()
    tiles = raster.debug_buffer("tiles_count")[:n]
    print(f"\n[pose-only kernel {name}] seed {seed} |ref|/S {(ref.abs() / S).tolist()} err/S {(err / S).tolist()} rows {int(got[6])} of {n}")
    assert bool((S > 0).all())
    assert bool((err <= 2e-5 * S).all()), (err / S).tolist()
    assert float(got[6]) == float((tiles != 0).sum()) > 0 and float(got[7]) == 0.0
    scratch = raster.debug_buffer("grad_scratch")
    assert scratch.numel() == 16 * n and not bool(scratch.view(torch.int32).any())        # every bit of every row
    with pytest.raises(RuntimeError, match="no backward context"):
        raster.compact_gradient_rows(act, torch.empty((n, 16), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    # the next forward is accepted, and its plain backward starts from zero rows without a clear
    raster.set_pose_gradient(None)
    rgba, dist, _, _ = raster.trace(*args)
    again, _ = raster.trace_bwd(*args, rgba, cot, dist, None)
    assert torch.allclose(again, dense, rtol=1e-3, atol=1e-4 * float(dense.abs().max()))


def test_a_forward_on_the_models_own_tensors_is_followed_too():
    """After a *_fields forward the rows are the ones that forward packed: particle_density is the row count."""
    sc = scenes.scene_c1(257, 0)
    act, sph = _rows(sc)
    view = make_view("pinhole", 128, 128, cams.look_at_c2w(*LOOK_AT))
    args = _trace_args(view, act, sph)
    raster, other = tracer_mod.SplatRaster({"render": {}}), tracer_mod.SplatRaster({"render": {}})
    out8, ref8 = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    other.set_pose_gradient(ref8)
    rgba, dist, _, _ = other.trace(*args)
    cot = _cotangent(rgba, 0)
    other.trace_bwd_pose(*_pose_args(args), rgba, cot, dist, None)
    raster.set_pose_gradient(out8)
    rgba, dist, _, _ = raster.trace_fields(0, 3, act[:, 0:3].contiguous(), act[:, 3:4].contiguous(), act[:, 4:8].contiguous(),
                                           act[:, 8:11].contiguous(), sph, *args[4:6], *args[7:12])
    raster.trace_bwd_pose(0, 3, 257, *args[4:6], *args[7:12], rgba, cot, dist, None)
    assert float(out8[6]) == float(ref8[6]) > 0
    assert torch.allclose(out8[:6], ref8[:6], rtol=1e-3, atol=1e-4 * float(ref8[:6].abs().max()))


# ---- 2. edges ----
def test_a_camera_that_sees_nothing_and_an_empty_scene_give_exact_zeros():
    sc = scenes.scene_c1(1000, 0)
    act, sph = _rows(sc)
    raster = tracer_mod.SplatRaster({"render": {}})
    out8 = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    raster.set_pose_gradient(out8)
    away = make_view("pinhole", 128, 128, cams.look_at_c2w((0.3, -0.2, -4.0), (0.3, -0.2, -9.0)))   # the scene is behind the camera
    args = _trace_args(away, act, sph)
    rgba, dist, _, _ = raster.trace(*args)
    raster.trace_bwd_pose(*_pose_args(args), rgba, torch.ones_like(rgba), dist, None)
    assert int((raster.debug_buffer("tiles_count")[:1000] != 0).sum()) == 0
    assert out8.tolist() == [0.0] * 8
    out8.fill_(float("nan"))
    args = _trace_args(make_view("pinhole", 128, 128, cams.look_at_c2w(*LOOK_AT)), act[:0].contiguous(), sph[:0].contiguous())
    rgba, dist, _, _ = raster.trace(*args)
    raster.trace_bwd_pose(*_pose_args(args), rgba, torch.ones_like(rgba), dist, None)
    assert out8.tolist() == [0.0] * 8


# ---- 3. refusals ----
def test_refusals_queue_nothing_and_the_handle_goes_on():
    sc = scenes.scene_c1(257, 0)
    act, sph = _rows(sc)
    view = make_view("pinhole", 64, 64, cams.look_at_c2w(*LOOK_AT))
    raster = tracer_mod.SplatRaster({"render": {}})
    args = _trace_args(view, act, sph)
    out8 = torch.full((8,), 7.0, dtype=torch.float32, device=DEV)

    def works():
        """the handle accepts the next forward and a pose-only backward reduces as usual"""
        raster.set_pose_gradient(out8)
        rgba, dist, _, _ = raster.trace(*args)
        raster.trace_bwd_pose(*_pose_args(args), rgba, torch.ones_like(rgba), dist, None)
        ok = bool(torch.isfinite(out8).all()) and float(out8[6]) > 0
        out8.fill_(7.0)
        return ok

    # no pose output set
    rgba, dist, _, _ = raster.trace(*args)
    with pytest.raises(RuntimeError, match="no pose output is set"):
        raster.trace_bwd_pose(*_pose_args(args), rgba, torch.ones_like(rgba), dist, None)
    with pytest.raises(RuntimeError, match="no backward context"):       # and no backward context came into being
        raster.compact_gradient_rows(act, torch.empty((257, 16), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    assert works()
    # a view with two poses
    raster.set_pose_gradient(out8)
    end = np.array(view["tq"], np.float32).copy()
    end[0] += np.float32(0.01)
    two = _trace_args(view, act, sph, pose_end=end)
    rgba, dist, _, _ = raster.trace(*two)
    with pytest.raises(RuntimeError, match="start and end poses differ"):
        raster.trace_bwd_pose(*_pose_args(two), rgba, torch.ones_like(rgba), dist, None)
    torch.cuda.synchronize()
    assert out8.tolist() == [7.0] * 8                                     # nothing was queued
    assert works()
    # arguments that differ from the cached forward
    rgba, dist, _, _ = raster.trace(*args)
    with pytest.raises(RuntimeError, match="differ from the cached forward"):
        raster.trace_bwd_pose(0, 3, act[:200].contiguous(), *_pose_args(args)[3:], rgba, torch.ones_like(rgba), dist, None)
    torch.cuda.synchronize()
    assert out8.tolist() == [7.0] * 8
    assert works()


def test_a_call_after_the_early_optimiser_pass_is_refused_and_the_fused_optimiser_has_nothing_to_follow():
    sc = scenes.scene_c1(1000, 0)
    view = make_view("pinhole", 128, 128, cams.look_at_c2w(*LOOK_AT))
    batch = to_batch(view, DEV)
    st = native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), gut.Tracer({"render": {}}), overlap_optimizer=True)
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    out8 = torch.full((8,), 7.0, dtype=torch.float32, device=DEV)
    st.raster.set_pose_gradient(out8)
    rgba, dist, _, _ = st.forward(batch)
    _, sensor, poses, _, _ = st._ctx
    pargs = (0, 3, st.act, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(), sensor, poses.timestamps_us[0], poses.timestamps_us[1],
             poses.T_world_sensors[0], poses.T_world_sensors[1], rgba, torch.ones_like(rgba), dist, None)
    st.raster.optimize_rows_without_gradient(*st._state(), *st._adam_settings(), st.act, lazy=st._lazy())
    with pytest.raises(RuntimeError, match="gut_optimize_rows_without_gradient was called for this forward"):
        st.raster.trace_bwd_pose(*pargs)
    torch.cuda.synchronize()
    assert out8.tolist() == [7.0] * 8
    st.raster.finish_optimizer_step_without_gradient()                   # ends the half-applied step; then the handle goes on
    rgba, dist, _, _ = st.forward(batch)
    st.raster.trace_bwd_pose(*pargs[:10], rgba, torch.ones_like(rgba), dist, None)
    assert bool(torch.isfinite(out8).all()) and float(out8[6]) > 0
    with pytest.raises(RuntimeError, match="no backward context"):
        st.raster.optimize_after_bwd(3, None, *st._state(), st.lr12, st.lr48, st.betas, st.eps, 1)
    st.raster.set_pose_gradient(None)
    st.forward(batch)                                                     # accepted


# ---- 4.-7. evaluate(pose_aligned=...) ----
@pytest.fixture(scope="module")
def held_out():
    """scene_c1(1000), four orbit views at 128 x 128, targets rendered at the TRUE poses; every given pose is off by a twist of 0.01 rad
    and 0.02 in centre position.  Shared by the tests below, which leave it unchanged."""
    sc = scenes.scene_c1(1000, 0)
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    rng = np.random.default_rng(11)
    true, exact, given = [], [], []
    for v in _orbit_batches(4):
        b = to_batch(v, DEV)
        with torch.no_grad():
            b.rgb_gt = tracer.render(model, b, train=False)["pred_rgb"].contiguous()
        c2w = np.asarray(v["c2w"], np.float64)
        true.append(c2w)
        exact.append(b)
        d_pos, d_rot = rng.standard_normal(3), rng.standard_normal(3)
        twist = np.concatenate([P_POS * d_pos / np.linalg.norm(d_pos), P_ROT * d_rot / np.linalg.norm(d_rot)])
        g = copy.copy(b)
        g.T_to_world = torch.as_tensor(pose.apply_pose_increment(c2w, twist), dtype=torch.float32)[None]
        given.append(g)
    return dict(model=model, tracer=tracer, true=true, exact=exact, given=given)


def test_perturbed_held_out_poses_are_recovered_with_the_model_frozen(held_out):
    """The set-up and the bar of test_perturbed_poses_are_recovered_with_the_gaussians_frozen, on held-out views through
    evaluate(pose_aligned=...): rates p / 20, 60 iterations; Adam moves a coordinate by about one rate per step, so a correct gradient
    arrives within 20 iterations and then stays within a few rates.  Every view's centre and rotation error against the true pose must
    end below its start and their means below p / 2; the aligned loss is at most the given one and the aligned PSNR above the plain
    one; the model's tensors are untouched; the plain metrics are those of evaluate without the option, bit for bit."""
    model, tracer, true, given = held_out["model"], held_out["tracer"], held_out["true"], held_out["given"]
    raw0, feat0 = model.raw.clone(), model.features.clone()
    plain = evaluate_mod.evaluate(model, tracer, given)
    res = evaluate_mod.evaluate(model, tracer, given, pose_aligned=RECOVERY)
    start = [pose.pose_difference(b.T_to_world.reshape(4, 4).double().numpy(), t) for b, t in zip(given, true)]
    end = [pose.pose_difference(np.asarray(p), t) for p, t in zip(res["pa_poses"], true)]
    print(f"\n[pose alignment] centre error start {[round(s[0], 5) for s in start]} end {[round(e[0], 5) for e in end]}\n"
          f"                 rotation error start {[round(s[1], 5) for s in start]} end {[round(e[1], 5) for e in end]}\n"
          f"                 psnr {[round(x, 2) for x in res['psnr']]} -> {[round(x, 2) for x in res['pa_psnr']]} "
          f"best iteration {res['pa_best_iteration']} loss {res['pa_loss_given']} -> {res['pa_loss_aligned']}")
    assert torch.equal(model.raw, raw0) and torch.equal(model.features, feat0)
    for k in ("psnr", "ssim", "mse", "l1", "mean_psnr", "std_psnr", "mean_ssim"):
        assert res[k] == plain[k], k
    assert "pa_psnr" not in plain and "pa_cc_psnr" not in res
    for s, e in zip(start, end):
        assert s[0] == pytest.approx(P_POS, rel=1e-3) and s[1] == pytest.approx(P_ROT, rel=1e-3)
        assert e[0] < s[0] and e[1] < s[1], (s, e)
    assert np.mean([e[0] for e in end]) < P_POS / 2 and np.mean([e[1] for e in end]) < P_ROT / 2
    for i in range(4):
        assert res["pa_loss_aligned"][i] <= res["pa_loss_given"][i]
        assert res["pa_psnr"][i] > res["psnr"][i]
        assert 0 < res["pa_best_iteration"][i] <= 60
    assert len(res["pa_poses"]) == 4 and np.asarray(res["pa_poses"]).shape == (4, 4, 4)
    assert res["mean_pa_psnr"] == pytest.approx(np.mean(res["pa_psnr"])) and res["std_pa_psnr"] == pytest.approx(np.std(res["pa_psnr"]))
    assert res["mean_pa_ssim"] == pytest.approx(np.mean(res["pa_ssim"]))
    assert res["mean_pa_translation"] == pytest.approx(np.mean(res["pa_translation"])) and res["mean_pa_translation"] > 0
    assert res["mean_pa_rotation_deg"] == pytest.approx(np.mean(res["pa_rotation_deg"])) and res["mean_pa_rotation_deg"] > 0
    assert len(res["pa_mse"]) == len(res["pa_l1"]) == len(res["pa_ssim"]) == 4
    assert getattr(tracer.tracer_wrapper, "_pose_out", None) is None       # what the handle had before: nothing


def test_a_view_given_at_its_true_pose_stays_there(held_out):
    res = evaluate_mod.evaluate(held_out["model"], held_out["tracer"], held_out["exact"][:2], pose_aligned=RECOVERY)
    for p, t, given, aligned in zip(res["pa_poses"], held_out["true"], res["pa_loss_given"], res["pa_loss_aligned"]):
        d = pose.pose_difference(np.asarray(p), t)
        assert d[0] < P_POS / 2 and d[1] < P_ROT / 2, d
        assert aligned <= given


def test_a_photo_no_pose_explains_stays_finite_and_zero_iterations_change_nothing(held_out):
    b = copy.copy(held_out["given"][0])
    b.rgb_gt = torch.rand((1, 128, 128, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    res = evaluate_mod.evaluate(held_out["model"], held_out["tracer"], [b], pose_aligned=dict(RECOVERY, iterations=20))
    flat = [res[k][0] for k in ("pa_psnr", "pa_ssim", "pa_mse", "pa_l1", "pa_translation", "pa_rotation_deg", "pa_loss_given", "pa_loss_aligned")]
    assert np.isfinite(flat).all() and np.isfinite(np.asarray(res["pa_poses"])).all()
    assert res["pa_loss_aligned"][0] <= res["pa_loss_given"][0]
    res = evaluate_mod.evaluate(held_out["model"], held_out["tracer"], [b, held_out["given"][1]], pose_aligned=dict(RECOVERY, iterations=0))
    for k in ("psnr", "ssim", "mse", "l1"):
        assert res["pa_" + k] == res[k], k                                 # the given pose bit for bit, so the same render and score
    assert res["pa_best_iteration"] == [0, 0] and res["pa_translation"] == [0.0, 0.0] and res["pa_loss_aligned"] == res["pa_loss_given"]
    for p, g in zip(res["pa_poses"], [b, held_out["given"][1]]):
        assert np.array_equal(np.asarray(p), g.T_to_world.reshape(4, 4).double().cpu().numpy())


def test_with_colour_correction_the_aligned_views_are_scored_corrected_too(held_out, tmp_path):
    gain = torch.tensor([1.2, 0.9, 1.1], device=DEV)
    views = []
    for g in held_out["given"][:2]:
        b = copy.copy(g)
        b.rgb_gt = (g.rgb_gt * gain).contiguous()
        views.append(b)
    res = evaluate_mod.evaluate(held_out["model"], held_out["tracer"], views, out_dir=str(tmp_path), step=7, colour_corrected=True,
                                pose_aligned=dict(RECOVERY, iterations=20))
    for k in ("pa_cc_psnr", "pa_cc_ssim", "pa_cc_mse", "pa_cc_l1"):
        assert len(res[k]) == 2 and np.isfinite(res[k]).all(), k
    assert res["mean_pa_cc_psnr"] == pytest.approx(np.mean(res["pa_cc_psnr"])) and res["std_pa_cc_psnr"] == pytest.approx(np.std(res["pa_cc_psnr"]))
    assert res["mean_pa_cc_ssim"] == pytest.approx(np.mean(res["pa_cc_ssim"]))
    assert res["mean_pa_cc_psnr"] >= res["mean_pa_psnr"]                   # the ridge property: corrected MSE <= plain MSE, per view
    assert all(c <= p for c, p in zip(res["pa_cc_mse"], res["pa_mse"]))
    assert "cc_psnr" in res and "cc_transforms" in res
    for sub in ("renders", "renders_cc", "renders_pa"):
        assert sorted(os.listdir(tmp_path / "ours_7" / sub)) == ["00000.png", "00001.png"], sub


# ---- 8. on a live trainer ----
def test_an_aligned_evaluation_between_two_train_steps_leaves_the_stepper_as_it_was(held_out):
    sc = scenes.scene_c1(1000, 0)
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    st = native.NativeTrainStep(model, tracer, pose_gradient=True)
    batch = copy.copy(held_out["exact"][0])
    batch.rgb_gt = torch.rand((1, 128, 128, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    st.step(batch)
    assert st.raster._pose_out is st.pose_gradient
    res = evaluate_mod.evaluate(model, tracer, held_out["given"][1:3], pose_aligned=dict(RECOVERY, iterations=5))
    assert len(res["pa_psnr"]) == 2
    assert st.raster._pose_out is st.pose_gradient                        # the stepper's buffer is the handle's output again
    scratch = st.raster.debug_buffer("grad_scratch")                      # before the second step: its backward will queue no clear
    assert scratch.numel() == 16 * 1000 and not bool(scratch.view(torch.int32).any())
    st.pose_gradient.fill_(float("nan"))
    st.step(batch)
    got = st.pose_gradient.cpu()
    assert bool(torch.isfinite(got).all()) and float(got[6]) > 0 and bool(got[:6].any())
    assert bool(torch.isfinite(model.raw).all())


# ---- 9. the command line ----
def test_cli_run_reports_the_aligned_means_and_writes_the_aligned_renders(tmp_path):
    scene = write_synthetic_colmap(str(tmp_path / "scene"), n_views=16, size=160, n_teacher=40_000, n_points=4_000)
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, "-m", "3dgrut_amd.trainer", "--path", scene, "--n-iterations", "60", "--out-dir", out,
                        "--refine-poses", "--aligned-metrics", "--align-iterations", "20"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    test = last["test"]
    for k in ("mean_pa_psnr", "std_pa_psnr", "mean_pa_ssim", "mean_pa_translation", "mean_pa_rotation_deg", "mean_psnr", "std_psnr",
              "mean_ssim", "n_views"):
        assert k in test and np.isfinite(test[k]), k
    assert not any(k.startswith("mean_pa_cc") for k in test)
    renders = sorted(os.listdir(os.path.join(out, "ours_60", "renders_pa")))
    assert len(renders) == test["n_views"] == len(os.listdir(os.path.join(out, "ours_60", "renders")))
