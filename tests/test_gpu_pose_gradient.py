"""The pose-gradient reduction on the GPU (gut_set_pose_gradient): the kernel against its float64 definition on the rows the same
backward returned, the rejection of views with two poses, the train step's output on its update paths, and the recovery of
perturbed poses with the Gaussians frozen."""
import importlib

import numpy as np
import pytest
import torch

from tests.common import FISHEYE_DIST, cams, make_view, pose, scenes, to_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
gut = importlib.import_module("3dgrut_amd")
tracer_mod = importlib.import_module("3dgrut_amd.tracer")
native = importlib.import_module("3dgrut_amd.native")
pose_refine = importlib.import_module("3dgrut_amd.pose_refine")

LOOK_AT = ((0.3, -0.2, -4.0), (0.0, 0.0, 0.0))


def _rows(sc):
    act = np.zeros((sc["positions"].shape[0], 12), np.float32)
    act[:, 0:3], act[:, 3:4], act[:, 4:8], act[:, 8:11] = sc["positions"], sc["density"], sc["rotation"], sc["scale"]
    return torch.as_tensor(act, device=DEV), torch.as_tensor(np.ascontiguousarray(sc["features"], np.float32), device=DEV)


def _trace_args(view, act, sph, pose_end=None):
    batch = to_batch(view, DEV)
    sensor, poses = tracer_mod.Tracer.create_camera_parameters(batch)
    tq0, tq1 = poses.T_world_sensors[0], poses.T_world_sensors[1] if pose_end is None else pose_end
    return (0, 3, act, sph, batch.rays_ori, batch.rays_dir, None, sensor, poses.timestamps_us[0], poses.timestamps_us[1], tq0, tq1)


def _backward_with_pose_gradient(raster, view, act, sph, seed):
    """Forward, then the plain gut_trace_bwd with a random cotangent while the pose output is set.  Returns (out8, dense [N,12]
    gradient of the same call, tiles_count)."""
    args = _trace_args(view, act, sph)
    out8 = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    raster.set_pose_gradient(out8)
    rgba, dist, _, _ = raster.trace(*args)
    cot = torch.as_tensor(np.random.default_rng(seed).standard_normal(tuple(rgba.shape)).astype(np.float32), device=DEV)
    dens_g, _ = raster.trace_bwd(*args, rgba, cot, dist, None)
    tiles = raster.debug_buffer("tiles_count")[:act.shape[0]] if act.shape[0] else torch.zeros(0, dtype=torch.int32, device=DEV)
    raster.set_pose_gradient(None)
    return out8.cpu().double(), dens_g, tiles


CASES = {
    "pinhole_128": dict(n=1000, kind="pinhole", W=128, H=128),
    "fisheye_144x96": dict(n=1000, kind="fisheye", W=144, H=96, distortion=FISHEYE_DIST),
    "pinhole_64_k16": dict(n=1000, kind="pinhole", W=64, H=64, k_buffer=16),
    "n257": dict(n=257, kind="pinhole", W=128, H=128),
    "n63": dict(n=63, kind="pinhole", W=128, H=128),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_definition_on_the_rows_of_the_same_backward(name):
    """|got_k - ref_k| <= 1e-5 S_k with S_k = sum_i |term_ik|: fp32 blocked summation of at most 2^20 terms plus a few ulps per
    term.  ref: pose_gradient_from_rows in float64 on the dense [N,12] gradient the same gut_trace_bwd returned — rows the epilogue
    read AFTER the reduction ran, so they also show that the reduction left them intact.  The cotangent seed is the first of
    0, 1, ... for which the reference alone says |ref_k| >= 1e-3 S_k for every k (otherwise the bar would be vacuous).  Slot 6 is
    the number of rows with a tile (the kernel does not skip unwalked waves), slot 7 is 0."""
    c = CASES[name]
    sc = scenes.scene_c1(c["n"], 0)
    act, sph = _rows(sc)
    view = make_view(c["kind"], c["W"], c["H"], cams.look_at_c2w(*LOOK_AT), distortion=c.get("distortion"))
    raster = tracer_mod.SplatRaster({"render": {"splat": {"k_buffer_size": c.get("k_buffer", 0)}}})
    cam_pos = np.asarray(view["c2w"], np.float64)[:3, 3]
    for seed in range(8):
        out8, dens_g, tiles = _backward_with_pose_gradient(raster, view, act, sph, seed)
        terms = pose.pose_gradient_terms(act, dens_g, cam_pos)
        ref, S = terms.sum(0).cpu(), terms.abs().sum(0).cpu()
        if bool((ref.abs() >= 1e-3 * S).all()):
            break
    else:
        pytest.fail(f"{name}: no cotangent seed below 8 gives |ref_k| >= 1e-3 S_k for every k")
    err = (out8[:6] - ref).abs()
    print(f"\n[pose kernel {name}] seed {seed} ref {ref.tolist()} |ref|/S {(ref.abs() / S).tolist()} err/S {(err / S).tolist()} "
          f"rows {int(out8[6])} of {act.shape[0]}")
    assert bool((S > 0).all())
    assert bool((err <= 1e-5 * S).all()), (err / S).tolist()
    assert float(out8[6]) == float((tiles != 0).sum()) > 0 and float(out8[7]) == 0.0


def test_a_camera_that_sees_nothing_and_an_empty_scene_give_exact_zeros():
    sc = scenes.scene_c1(1000, 0)
    act, sph = _rows(sc)
    raster = tracer_mod.SplatRaster({"render": {}})
    away = make_view("pinhole", 128, 128, cams.look_at_c2w((0.3, -0.2, -4.0), (0.3, -0.2, -9.0)))   # the scene is behind the camera
    out8, dens_g, tiles = _backward_with_pose_gradient(raster, away, act, sph, 0)
    assert int((tiles != 0).sum()) == 0 and not bool(dens_g.any())
    assert out8.tolist() == [0.0] * 8
    empty_act, empty_sph = act[:0].contiguous(), sph[:0].contiguous()
    out8, dens_g, _ = _backward_with_pose_gradient(raster, make_view("pinhole", 128, 128, cams.look_at_c2w(*LOOK_AT)), empty_act, empty_sph, 0)
    assert tuple(dens_g.shape) == (0, 12)
    assert out8.tolist() == [0.0] * 8


def test_a_view_with_two_poses_is_refused_and_the_handle_goes_on():
    sc = scenes.scene_c1(257, 0)
    act, sph = _rows(sc)
    view = make_view("pinhole", 64, 64, cams.look_at_c2w(*LOOK_AT))
    raster = tracer_mod.SplatRaster({"render": {}})
    out8 = torch.full((8,), 7.0, dtype=torch.float32, device=DEV)
    raster.set_pose_gradient(out8)
    end = np.array(view["tq"], np.float32).copy()
    end[0] += np.float32(0.01)                            # the end pose differs from the start pose
    args = _trace_args(view, act, sph, pose_end=end)
    rgba, dist, _, _ = raster.trace(*args)
    with pytest.raises(RuntimeError, match="start and end poses differ"):
        raster.trace_bwd(*args, rgba, torch.ones_like(rgba), dist, None)
    torch.cuda.synchronize()
    assert out8.tolist() == [7.0] * 8                     # nothing was queued
    # the handle accepts the next forward, and a one-pose view reduces as usual
    got, dens_g, _ = _backward_with_pose_gradient(raster, view, act, sph, 1)
    assert bool(torch.isfinite(got).all()) and float(got[6]) > 0
    # with the output off the same two-pose view is differentiated as before
    rgba, dist, _, _ = raster.trace(*args)
    dens_g, _ = raster.trace_bwd(*args, rgba, torch.ones_like(rgba), dist, None)
    assert bool(dens_g.any())
    with pytest.raises(RuntimeError, match="8 elements"):
        raster.set_pose_gradient(torch.zeros(6, device=DEV))


def _orbit_batches(n_views, size=128, radius=4.0):
    out = []
    for i in range(n_views):
        c2w = cams.orbit_c2w(radius, 360.0 * i / n_views, 10.0 + 20.0 * (i % 3) / 2.0)
        out.append(make_view("pinhole", size, size, c2w))
    return out


STEP_PATHS = {
    "one_pass": dict(overlap_optimizer=False),
    "one_pass_overlap": dict(overlap_optimizer=True),          # the side stream updates rows while the reduction runs
    "unfused": dict(fused_sh_adam=False),
    "sparse_exchange": dict(fuse_epilogue=False, dp_exchange="sparse", overlap_optimizer=False),   # gut_compact_gradient_rows
    "dense_exchange": dict(fuse_epilogue=False, dp_exchange="dense", overlap_optimizer=False),     # the compact epilogue
}


@pytest.mark.parametrize("path", list(STEP_PATHS))
def test_train_step_leaves_the_pose_gradient_of_its_view(path):
    """NativeTrainStep(pose_gradient=True) on its update paths against the definition, evaluated on the dense gradient a plain
    backward of a second handle returns for the same rows and the same d loss / d rgba.  Bar 2e-5 S_k: 1e-5 S_k for the reduction
    (as above) and as much again for the rows themselves, which the two backwards accumulate with float atomics in different orders."""
    sc = scenes.scene_c1(1000, 0)
    view = make_view("pinhole", 128, 128, cams.look_at_c2w(*LOOK_AT))
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, 128, 128, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), pose_gradient=True, **STEP_PATHS[path])
    assert tuple(st.pose_gradient.shape) == (8,) and st.pose_gradient.is_cuda
    act, feat = st.activate().clone(), model.features.clone()   # what the step's forward reads (the step then updates both)
    captured = {}
    loss_fn = st._loss

    def capture(b, rgba):
        out = loss_fn(b, rgba)
        captured["rgba_grad"] = out[2].clone()
        return out
    st._loss = capture
    st.step(batch)
    got = st.pose_gradient.cpu().double()
    other = tracer_mod.SplatRaster({"render": {}})
    args = _trace_args(view, act, feat)
    rgba, dist, _, _ = other.trace(*args)
    dens_g, _ = other.trace_bwd(*args, rgba, captured["rgba_grad"], dist, None)
    terms = pose.pose_gradient_terms(act, dens_g, np.asarray(view["c2w"], np.float64)[:3, 3])
    ref, S = terms.sum(0).cpu(), terms.abs().sum(0).cpu()
    err = (got[:6] - ref).abs()
    print(f"\n[pose step {path}] ref {ref.tolist()} err/S {(err / S).tolist()} rows {int(got[6])}")
    assert bool((ref.abs() >= 1e-3 * S).all()), (ref.abs() / S).tolist()
    assert bool((err <= 2e-5 * S).all()), (err / S).tolist()
    assert float(got[6]) == float((other.debug_buffer("tiles_count")[:1000] != 0).sum())
    off = native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), gut.Tracer({"render": {}}))
    assert off.pose_gradient is None


def test_the_output_can_be_switched_off_between_steps():
    """enable_pose_gradient(False): the next backward launches nothing for it (the buffer keeps what it held, the handle's output is
    cleared); on again, the step fills it as before."""
    sc = scenes.scene_c1(257, 0)
    view = make_view("pinhole", 64, 64, cams.look_at_c2w(*LOOK_AT))
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, 64, 64, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    st = native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), gut.Tracer({"render": {}}), pose_gradient=True)
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    buf = st.pose_gradient
    st.step(batch)
    first = buf.clone()
    assert float(first[6]) > 0 and bool(first[:6].any())
    st.enable_pose_gradient(False)
    assert st.pose_gradient is None and st.raster._pose_out is None
    buf.fill_(3.0)
    st.step(batch)
    assert buf.tolist() == [3.0] * 8
    st.enable_pose_gradient(True)
    st.step(batch)
    assert st.pose_gradient is buf and float(buf[6]) == float(first[6])
    assert torch.allclose(buf[:6], first[:6], rtol=1e-3, atol=1e-4 * float(first[:6].abs().max()))   # the same frozen scene and view
    with pytest.raises(ValueError, match="without pose_gradient"):
        native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), gut.Tracer({"render": {}})).enable_pose_gradient(True)
    cpu = pose_refine.PoseRefiner([torch.eye(4)], "cpu", 1e-3, 5e-4)
    with pytest.raises(ValueError, match="the gradient is on"):
        cpu.end(0, buf)
    dev = pose_refine.PoseRefiner([torch.eye(4)] * 3, DEV, 1e-3, 5e-4)
    assert all(dev._slots[v].is_pinned() for v in range(3))   # the copies into the slots do not block the host


def test_pose_adam_kernel_equals_the_host_arithmetic():
    """gut_pose_adam_step against PoseRefiner's host-tensor form over three visits of one view: the same fp32 operations, so a
    few ulps (powf and the division may round differently: 1e-6 relative)."""
    cpu = pose_refine.PoseRefiner([torch.eye(4)] * 2, "cpu", 1e-3, 5e-4)
    dev = pose_refine.PoseRefiner([torch.eye(4)] * 2, DEV, 1e-3, 5e-4)
    rng = np.random.default_rng(2)
    for visit in range(3):
        g = torch.zeros(8)
        g[:6] = torch.as_tensor(rng.standard_normal(6) * 10.0 ** rng.integers(-3, 3), dtype=torch.float32)
        for r, grad in ((cpu, g), (dev, g.to(DEV))):
            r.end(1, grad)
            r._apply_pending(1)
        torch.cuda.synchronize()
        assert dev.counts.tolist() == [0, visit + 1] == cpu.counts.tolist()
        assert torch.allclose(dev.m.cpu(), cpu.m, rtol=1e-6, atol=0) and torch.allclose(dev.v.cpu(), cpu.v, rtol=1e-6, atol=0)
        assert torch.allclose(dev._slots, cpu._slots, rtol=1e-5, atol=0)
        assert not dev.m[0].any() and not dev._slots[0].any()
    assert np.allclose(dev.poses, cpu.poses, rtol=0, atol=1e-9)


def test_perturbed_poses_are_recovered_with_the_gaussians_frozen():
    """scene_c1(1000), eight orbit views at 128 x 128 whose targets the library rendered at the TRUE poses; every training pose is
    off by a known twist of size p = 0.01 rad and 0.02 in centre position (under two pixels).  All Gaussian learning rates are 0 and
    there is no regulariser, so only the poses can move; pose rates p / 20, 60 visits per view.  Adam moves a coordinate by about one
    rate per step, so a correct gradient arrives within 20 visits and then stays within a few rates: every view's rotation error and
    centre error must end below their start, and their means below p / 2."""
    P_ROT, P_POS, VISITS = 0.01, 0.02, 60
    sc = scenes.scene_c1(1000, 0)
    views = _orbit_batches(8)
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    st = native.NativeTrainStep(model, tracer, pose_gradient=True)
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    raw0, feat0 = model.raw.clone(), model.features.clone()
    rng = np.random.default_rng(11)
    true, batches = [], []
    for v in views:
        b = to_batch(v, DEV)
        with torch.no_grad():
            b.rgb_gt = tracer.render(model, b, train=False)["pred_rgb"].contiguous()
        c2w = np.asarray(v["c2w"], np.float64)
        true.append(c2w)
        d_pos, d_rot = rng.standard_normal(3), rng.standard_normal(3)
        twist = np.concatenate([P_POS * d_pos / np.linalg.norm(d_pos), P_ROT * d_rot / np.linalg.norm(d_rot)])
        b.T_to_world = torch.as_tensor(pose.apply_pose_increment(c2w, twist), dtype=torch.float32)[None]
        batches.append(b)
    refiner = pose_refine.PoseRefiner([b.T_to_world for b in batches], DEV, lr_translation=P_POS / 20, lr_rotation=P_ROT / 20)
    start = [pose.pose_difference(p, t) for p, t in zip(refiner.poses, true)]
    for _ in range(VISITS):
        for i, b in enumerate(batches):
            st.step(refiner.begin(i, b))
            refiner.end(i, st.pose_gradient)
    end = [pose.pose_difference(p, t) for p, t in zip(refiner.refined_poses().numpy(), true)]
    print(f"\n[pose recovery] centre error start {[round(s[0], 5) for s in start]} end {[round(e[0], 5) for e in end]}\n"
          f"                rotation error start {[round(s[1], 5) for s in start]} end {[round(e[1], 5) for e in end]}")
    assert refiner.counts.tolist() == [VISITS] * 8
    assert torch.equal(model.raw, raw0) and torch.equal(model.features, feat0)        # the scene could not move
    for s, e in zip(start, end):
        assert s[0] == pytest.approx(P_POS, rel=1e-3) and s[1] == pytest.approx(P_ROT, rel=1e-3)
        assert e[0] < s[0] and e[1] < s[1], (s, e)
    assert np.mean([e[0] for e in end]) < P_POS / 2 and np.mean([e[1] for e in end]) < P_ROT / 2
    # with the refiner off the poses do not change: the step neither reads nor writes a pose
    given = [b.T_to_world.clone() for b in batches]
    off = native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), tracer)
    for b in batches:
        off.step(b)
    assert off.pose_gradient is None and all(torch.equal(b.T_to_world, g) for b, g in zip(batches, given))
