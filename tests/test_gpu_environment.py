"""The cube-map background on the GPU: the sampler and both forms of the adjoint bit for bit against the float32
restatement of tests/environment_reference.py, autograd through EnvironmentMap.sample, one train step on the fused branch against
the torch branch, the recovery of a known map with the Gaussians frozen, and a short trainer run with its resume."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import environment_reference as er
from tests.common import cams, make_view, rel_l2, scenes, to_batch
from tests.synthetic_colmap import load_scene, write_synthetic_colmap
from tests.test_cpu_environment import RECOVERY_R, recovery_coverage, recovery_views

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
_capi = importlib.import_module("3dgrut_amd._capi")
native = importlib.import_module("3dgrut_amd.native")
losses = importlib.import_module("3dgrut_amd.losses")
environment = importlib.import_module("3dgrut_amd.environment")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
evaluate = importlib.import_module("3dgrut_amd.evaluate").evaluate
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"
ALL = er.CASES + ("f",)
NAN = float("nan")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _view(rays, M):
    H, W = rays.shape[:2]
    return _capi.GutEnvironmentView(rays.data_ptr(), (C.c_float * 9)(*[float(x) for x in np.asarray(M, np.float32).reshape(9)]), H, W)


def _sample(rays, M, texels):
    """gut_environment_sample into a NaN-filled plane."""
    rays, texels = _dev(rays), _dev(texels)
    out = torch.full(tuple(rays.shape[:2]) + (3,), NAN, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(_capi.load().gut_environment_sample(C.c_void_p(stream), C.byref(_view(rays, M)), texels.data_ptr(), int(texels.shape[1]),
                                                    out.data_ptr()), "environment_sample")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _backward(rays, M, R, plane_grad=None, rgba=None, rgba_grad=None):
    """gut_environment_backward into a NaN-filled gradient, from a NaN-filled workspace."""
    lib = _capi.load()
    rays = _dev(rays)
    ts = [None if t is None else _dev(t) for t in (plane_grad, rgba, rgba_grad)]
    ws = torch.full(((lib.gut_environment_workspace_bytes(R) + 7) // 8,), -1, dtype=torch.int64, device=DEV)
    grad = torch.full((6, R, R, 3), NAN, dtype=torch.float32, device=DEV)
    cot = _capi.GutEnvironmentCotangent(*[None if t is None else t.data_ptr() for t in ts])
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.gut_environment_backward(C.c_void_p(stream), C.byref(_view(rays, M)), C.byref(cot), R, ws.data_ptr(), grad.data_ptr()),
                "environment_backward")
    torch.cuda.synchronize()
    return grad.cpu().numpy()


def _texels(R, seed=3):
    return np.random.default_rng(seed).standard_normal((6, R, R, 3)).astype(np.float32)


# ---- 1. the sampler ----
@pytest.mark.parametrize("name", ALL)
def test_sampler_bit_for_bit(name):
    """Every float of the plane equals the float32 restatement's; a zero and a NaN direction give +0.  `f` is a fisheye-style ray
    table, 40 x 40 over 180 degrees, that reaches at least five faces."""
    rays, M, R = er.case(name)
    rays = rays.copy()
    rays[0, 0], rays[3, 5, 1] = 0.0, np.nan
    T = _texels(R)
    got, ref = _sample(rays, M, T), er.sample32(rays, M, T)
    assert not np.isnan(got).any()
    assert not _bits(got[0, 0]).any() and not _bits(got[3, 5]).any()
    wrong = int((_bits(got) != _bits(ref)).sum())
    assert wrong == 0, f"{wrong} of {got.size} floats differ, max |difference| {np.abs(got - ref).max()}"
    if name == "f":
        assert len(set(er.taps32(rays, M, R)[1][er.taps32(rays, M, R)[0]].tolist())) >= 5


# ---- 2. the adjoint ----
def _cotangents(rays, seed):
    """(g [H,W,4] random signed with non-finite entries, rgba [H,W,4] with alpha in [0, 1] including exact 0 and 1)."""
    H, W = rays.shape[:2]
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((H, W, 4)).astype(np.float32)
    g[1, 2, 0], g[5, 7, 1], g[9, 3, 2], g[11, 13, 0] = np.nan, np.inf, -np.inf, np.nan
    rgba = rng.random((H, W, 4)).astype(np.float32)
    rgba[::4, ::3, 3], rgba[1::4, 1::3, 3] = 0.0, 1.0
    return g, rgba


@pytest.mark.parametrize("name", ALL)
def test_adjoint_bit_for_bit(name):
    """Both cotangent forms into a NaN-filled gradient: every element equals the int64 restatement, converted.  Case (b) has more
    distinct texels in one 16 x 16 pixel tile than kEnvSlots (the direct route runs), case (a) fewer (the LDS route runs).  As bits:
    two calls agree, grad(-c) = -grad(c), grad(2^m c) = 2^m grad(c)."""
    rays, M, R = er.case(name)
    rays = rays.copy()
    rays[2, 2] = 0.0                                  # a void pixel scatters nothing
    g, rgba = _cotangents(rays, 11)
    per_tile = er.distinct_texels_per_tile(rays, M, R)
    if name == "a":
        assert max(per_tile) < _capi.kEnvSlots
    if name == "b":
        assert min(per_tile) > _capi.kEnvSlots
    plane = np.ascontiguousarray(g[..., :3])
    ref_plane = er.adjoint32(rays, M, R, plane)
    got_plane = _backward(rays, M, R, plane_grad=plane)
    assert not np.isnan(got_plane).any()
    assert np.array_equal(_bits(got_plane), _bits(ref_plane)), np.abs(got_plane - ref_plane).max()
    ref_pair = er.adjoint32(rays, M, R, er.cotangent_from_rgba(rgba, g))
    got_pair = _backward(rays, M, R, rgba=rgba, rgba_grad=g)
    assert np.array_equal(_bits(got_pair), _bits(ref_pair)), np.abs(got_pair - ref_pair).max()
    assert np.abs(ref_pair).max() > 0 and not np.array_equal(ref_pair, ref_plane)
    # as bits
    assert np.array_equal(_bits(_backward(rays, M, R, plane_grad=plane)), _bits(got_plane))
    assert np.array_equal(_bits(_backward(rays, M, R, plane_grad=-plane)), _bits(np.float32(0) - got_plane))     # (0 - g: +0 stays +0)
    for m in (-20, 60):
        assert np.array_equal(_bits(_backward(rays, M, R, plane_grad=np.ldexp(plane, m))), _bits(np.ldexp(got_plane, m))), m
    assert not _bits(_backward(rays, M, R, plane_grad=np.zeros_like(plane))).any()


# ---- 3. autograd ----
def test_sample_under_autograd():
    """EnvironmentMap.sample under autograd gives the gradient bits of the plane form; with requires_grad off the plane's bits are
    unchanged and there is no graph."""
    rays, _, R = er.case("c")
    view = make_view("pinhole", 40, 40, cams.orbit_c2w(4.0, 40.0, 25.0))
    M = environment.rotation_from_pose(view["c2w"])
    env = environment.EnvironmentMap(R, 0.5, DEV)
    env.texels.copy_(_dev(_texels(R)))
    rays_dev, T = _dev(rays)[None], _dev(view["c2w"])[None]
    plain = env.sample(rays_dev, T)
    assert not plain.requires_grad and tuple(plain.shape) == (40, 40, 3)
    assert np.array_equal(_bits(plain), _bits(er.sample32(rays, M.reshape(3, 3), env.texels.cpu().numpy())))
    env.texels.requires_grad_(True)
    out = env.sample(rays_dev, T)
    assert out.requires_grad and np.array_equal(_bits(out), _bits(plain))
    c = torch.as_tensor(np.random.default_rng(5).standard_normal((40, 40, 3)).astype(np.float32), device=DEV)
    (out * c).sum().backward()
    assert np.array_equal(_bits(env.texels.grad), _bits(_backward(rays, M, R, plane_grad=c.cpu().numpy())))
    assert np.array_equal(_bits(env.texels.grad), _bits(er.adjoint32(rays, M.reshape(3, 3), R, c.cpu().numpy())))


# ---- 4. one train step ----
H, W = 64, 96


def _step_batch():
    # the view and shapes of tests/test_gpu_background_training.py
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.25, -0.1, -3.5), (0.25, 0.0, 0.0)), fx=110.0)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    return batch


def _one_step(sc, batch, fused_loss, env_texels):
    """One step of a fresh NativeTrainStep; env_texels None: no map, "unset": the attribute is never touched."""
    model = native.NativeGaussianModel(sc, device=DEV)
    if isinstance(env_texels, np.ndarray):
        model.environment = environment.EnvironmentMap(env_texels.shape[1], 0.5, DEV)
        model.environment.texels.copy_(_dev(env_texels))
    elif env_texels is None:
        model.environment = None
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fused_loss=fused_loss)
    seen, inner = [], st._loss
    st._loss = lambda b, rgba: (seen.append(rgba.clone()), seen.append(inner(b, rgba)), seen[-1])[2]
    loss, out = st.step(batch)
    torch.cuda.synchronize()
    return st, loss, out, seen[1][2], seen[0]


def test_one_step_fused_against_the_torch_branch():
    """Loss to 1e-5, rgba_grad and texels.grad to rel-L2 2e-5 (the one-step bounds of tests/test_gpu_background_training.py for the
    plane form); the map took its Adam step on both branches; the fused loss IS the background-plane loss over the map's plane."""
    sc = scenes.scene_c1(4000, 21)
    batch = _step_batch()
    T0 = (0.5 + 0.3 * _texels(8, seed=9)).astype(np.float32)
    fs, floss, fout, fgrad, rgba = _one_step(sc, batch, True, T0)
    ts, tloss, tout, tgrad, _ = _one_step(sc, batch, False, T0)
    fenv, tenv = fs.model.environment, ts.model.environment
    print(f"\n[environment step] loss fused {float(floss):.8f} torch {float(tloss):.8f}; rgba_grad rel-L2 "
          f"{rel_l2(fgrad.cpu().numpy(), tgrad.cpu().numpy()):.3e}; texels.grad rel-L2 {rel_l2(fenv.texels.grad.cpu().numpy(), tenv.texels.grad.cpu().numpy()):.3e}")
    assert abs(float(floss) - float(tloss)) <= 1e-5
    assert rel_l2(fgrad.cpu().numpy(), tgrad.cpu().numpy()) <= 2e-5
    assert float(fenv.texels.grad.abs().max()) > 0
    assert rel_l2(fenv.texels.grad.cpu().numpy(), tenv.texels.grad.cpu().numpy()) <= 2e-5
    for env in (fenv, tenv):
        moved = env.texels.cpu().numpy() != T0
        assert moved.any() and not (moved & (env.texels.grad.cpu().numpy() == 0)).any()      # Adam moves only what has a gradient
        assert not env.texels.requires_grad
    # the background did show through, and pred_rgb is the composite over the plane
    env0 = environment.EnvironmentMap(8, 0.5, DEV)
    env0.texels.copy_(_dev(T0))
    plane = env0.plane(batch).clone()
    assert float(plane.std()) > 0.05
    loss3, grad = losses.fused_photometric_loss(rgba, batch.rgb_gt, plane, 0.8, 0.2)
    assert float(loss3[0]) == float(floss) and torch.equal(grad, fgrad)
    assert torch.equal(fout["pred_rgb"][0], rgba[..., :3] + plane * (1.0 - rgba[..., 3:]))
    assert np.array_equal(_bits(fenv.texels.grad), _bits(_backward(batch.rays_dir[0].cpu().numpy(), environment.rotation_from_pose(batch.T_to_world),
                                                                    8, rgba=rgba.cpu().numpy(), rgba_grad=fgrad.cpu().numpy())))
    black = _one_step(sc, batch, True, None)[1]
    assert abs(float(black) - float(floss)) > 1e-3


def test_without_a_map_the_step_is_what_it_was():
    """environment = None set on the model against a model whose attribute was never touched: loss, pred_rgb and rgba_grad are
    bit-identical (the forward and the loss kernels are deterministic), and nothing of the map's is queued."""
    sc = scenes.scene_c1(4000, 21)
    batch = _step_batch()
    a = _one_step(sc, batch, True, None)
    b = _one_step(sc, batch, True, "unset")
    assert "environment" in vars(a[0].model) and "environment" not in vars(b[0].model)
    assert float(a[1]) == float(b[1]) and torch.equal(a[2]["pred_rgb"], b[2]["pred_rgb"]) and torch.equal(a[3], b[3])


# ---- 5. recovery ----
def _true_map():
    """0.5 + 0.4 (unit direction) per texel centre at R = 16, float64 [6,16,16,3]."""
    R = RECOVERY_R
    c = (np.arange(R) + 0.5) / (0.5 * R) - 1.0
    out = np.zeros((6, R, R, 3))
    for face in range(6):
        axis, sign = face // 2, (1.0 if face % 2 == 0 else -1.0)
        e = np.zeros((R, R, 3))
        e[..., axis] = sign
        e[..., (axis + 1) % 3] = c[None, :]          # u along the columns
        e[..., (axis + 2) % 3] = c[:, None]          # v along the rows
        out[face] = 0.5 + 0.4 * e / np.linalg.norm(e, axis=-1, keepdims=True)
    return out


def test_a_known_map_is_recovered_with_the_gaussians_frozen():
    """scene_c1(1000), the eight orbit views at 128 x 128 of tests/test_gpu_pose_gradient.py; the targets are the library's render
    composited over a smooth true map whose planes the float64 definition built on the CPU.  All Gaussian rates are 0, the map
    starts at 0.5, default lr (0.01), 60 visits per view.  Over the texels that receive sum_p (1 - alpha) w >= 1 (with the oracle's
    alpha: the precondition tests/test_cpu_environment.py counts), the mean |texel - true| ends below half its start, and no such
    texel ends worse than it started by more than 5 lr = 0.05: Adam moves a texel by about one rate per visit and, around its
    optimum, stays within a few rates of it, so a texel that started at its true value may end that far from it and no further."""
    sc = scenes.scene_c1(1000, 0)
    views = recovery_views()
    act = np.zeros((1000, 12), np.float32)
    act[:, 0:3], act[:, 3:4], act[:, 4:8], act[:, 8:11] = sc["positions"], sc["density"], sc["rotation"], sc["scale"]
    alphas = [oracle.forward(v["oracle_cam"], 128, 128, act, sc["features"], v["ro"], v["rd"])["rgba"][..., 3] for v in views]
    counted = recovery_coverage(alphas, views) >= 1.0
    assert int(counted.sum()) >= 100
    true = _true_map()
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    batches = []
    for v in views:
        b = to_batch(v, DEV)
        with torch.no_grad():
            out = tracer.render(model, b, train=False)
        M = environment.rotation_from_pose(v["c2w"]).reshape(3, 3)
        B = torch.as_tensor(er.sample64(v["rd"].reshape(128, 128, 3), M, true), device=DEV)
        b.rgb_gt = (out["pred_rgb"].double() + B[None] * (1.0 - out["pred_opacity"].double())).float().contiguous()
        batches.append(b)
    env = environment.EnvironmentMap(RECOVERY_R, 0.5, DEV)
    model.environment = env
    st = native.NativeTrainStep(model, tracer)
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    raw0, feat0 = model.raw.clone(), model.features.clone()
    start = np.abs(env.texels.cpu().numpy().astype(np.float64) - true).mean(-1)
    for visit in range(60):
        for b in batches:
            st.step(b)
    torch.cuda.synchronize()
    assert torch.equal(model.raw, raw0) and torch.equal(model.features, feat0)
    end = np.abs(env.texels.cpu().numpy().astype(np.float64) - true).mean(-1)
    worse = float((end - start)[counted].max())
    print(f"\n[environment recovery] {int(counted.sum())} texels: mean |texel - true| {start[counted].mean():.4f} -> {end[counted].mean():.4f}, "
          f"largest end - start {worse:.4f}")
    assert end[counted].mean() < 0.5 * start[counted].mean()
    assert worse <= 5 * 0.01


# ---- 6. the trainer ----
NO_EVENTS = dict(densify=dict(start_iteration=-1, end_iteration=-1), prune=dict(start_iteration=-1, end_iteration=-1),
                 reset_density=dict(start_iteration=-1, end_iteration=-1))


def _freeze(tr):
    """All Gaussian rates 0 and no schedule to bring the position rate back: only the map can move."""
    tr.stepper.schedule = None
    tr.stepper.lr12[:] = 0.0
    tr.stepper.lr48[:] = 0.0
    return tr


def test_trainer_run_with_resume(tmp_path):
    """A reduced synthetic COLMAP scene (16 views of 160 x 160, every 8th held out), the `environment` block at R = 32.

    40 steps with the default rates: the Gaussians and the map are learnt together; environment.npy, the statistics' keys and
    Trainer.environment() are there; evaluation composites the map for held-out views, and over a zero map the render is the
    black-background render, bit for bit.

    Resume: 40 steps straight against 20 steps, a checkpoint and a Trainer resumed from it — map and model bits are those of the
    uninterrupted run.  This pair runs with the Gaussians' rates at 0: the backward compositor sums the per-Gaussian gradients with
    float atomics, so two identical runs of this trainer WITHOUT a map already differ in the model's bits (measured on this scene: 20
    steps, largest |difference| of a raw parameter 4.4e-3), and bit identity of a continued run can only be stated of what is
    deterministic — the forward, the loss, the sampler, the adjoint, the map's Adam and the checkpoint's round trip, which is
    everything this feature adds.  With the default rates the resumed trainer restores the saved bits of map and model and runs on."""
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=16, size=160, n_teacher=40_000, n_points=4_000)
    init, tb, vb, extent = load_scene(root)
    conf = dict(n_iterations=40, val_frequency=10 ** 9, test_last=False, seed=0, environment=dict(enabled=True, resolution=32),
                checkpoint=dict(iterations=[20]), strategy=dict(method="GSStrategy", **NO_EVENTS))
    out = str(tmp_path / "learnt")
    learnt = trainer_mod.Trainer(dict(conf, out_dir=out), init, tb, test_batches=vb, scene_extent=extent)
    raw0 = learnt.model.raw.clone()
    stats = learnt.train()
    assert not torch.equal(learnt.model.raw, raw0)
    assert stats["environment_resolution"] == 32 and len(stats["environment_mean_colour"]) == 3
    assert json.loads(json.dumps(stats))["environment_mean_colour"] == stats["environment_mean_colour"]
    texels = learnt.environment()
    assert tuple(texels.shape) == (6, 32, 32, 3) and not texels.is_cuda
    assert np.array_equal(np.load(os.path.join(out, "environment.npy")), texels.numpy())
    assert bool((texels != 0.5).any())                                     # the map was learnt
    assert stats["environment_mean_colour"] == pytest.approx(texels.reshape(-1, 3).mean(0).tolist(), abs=1e-6)
    mid = os.path.join(out, "ours_20", "ckpt_20.pt")
    saved = torch.load(mid, map_location="cpu", weights_only=True)
    assert float(saved["native"]["environment"]["step"]) == 20.0
    again = trainer_mod.Trainer(dict(conf, out_dir="", resume=mid), None, tb, test_batches=vb, scene_extent=extent)
    assert again.global_step == 20 and torch.equal(again.environment(), saved["native"]["environment"]["texels"])
    assert torch.equal(again.model.raw[:, 0:3].cpu(), saved["positions"])
    again.train()
    assert again.global_step == 40 and bool(torch.isfinite(again.environment()).all())
    with pytest.raises(ValueError, match="resume with --environment"):
        trainer_mod.Trainer(dict(conf, out_dir="", resume=mid, environment=dict(enabled=False)), None, tb, scene_extent=extent)
    del again

    # the command line: main() parses the three flags
    out_c = str(tmp_path / "cli")
    assert trainer_mod.main(["--path", root, "--n-iterations", "5", "--out-dir", out_c, "--environment", "--environment-resolution", "8",
                             "--environment-lr", "0.02"]) == 0
    assert np.load(os.path.join(out_c, "environment.npy")).shape == (6, 8, 8, 3)
    assert set(torch.load(os.path.join(out_c, "ckpt_last.pt"), map_location="cpu", weights_only=True)["native"]["environment"]) == \
        {"texels", "exp_avg", "exp_avg_sq", "step"}

    # the resume, bit for bit, with the Gaussians frozen
    out_f = str(tmp_path / "frozen")
    straight = _freeze(trainer_mod.Trainer(dict(conf, out_dir=out_f), init, tb, test_batches=vb, scene_extent=extent))
    raw0, feat0 = straight.model.raw.clone(), straight.model.features.clone()
    straight.train()
    assert torch.equal(straight.model.raw, raw0) and torch.equal(straight.model.features, feat0)
    mid_f = os.path.join(out_f, "ours_20", "ckpt_20.pt")
    resumed = _freeze(trainer_mod.Trainer(dict(conf, out_dir="", resume=mid_f), None, tb, test_batches=vb, scene_extent=extent))
    assert resumed.global_step == 20
    assert torch.equal(resumed.environment(), torch.load(mid_f, map_location="cpu", weights_only=True)["native"]["environment"]["texels"])
    assert not torch.equal(resumed.environment(), straight.environment())
    resumed.train()
    assert torch.equal(resumed.environment(), straight.environment())
    assert torch.equal(resumed.model.raw, straight.model.raw) and torch.equal(resumed.model.features, straight.model.features)
    a, b = straight.environment_map.state_dict(), resumed.environment_map.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a) and float(a["step"]) == 40.0
    del straight, resumed

    # evaluation: the held-out views are rendered over the map
    env, model, tracer = learnt.environment_map, learnt.model, learnt.tracer
    with torch.no_grad():
        over = tracer.render(model, vb[0], train=False)
        model.environment = None
        black = tracer.render(model, vb[0], train=False)
        model.environment = env
        assert torch.equal(over["pred_rgb"][0], black["pred_rgb"][0] + env.plane(vb[0]) * (1.0 - black["pred_opacity"][0]))
        assert not torch.equal(over["pred_rgb"], black["pred_rgb"])
        with_map = evaluate(model, tracer, vb)["mean_psnr"]
        env.texels.zero_()
        zero = tracer.render(model, vb[0], train=False)
        assert torch.equal(zero["pred_rgb"], black["pred_rgb"]) and torch.equal(zero["pred_opacity"], black["pred_opacity"])
        over_zero = evaluate(model, tracer, vb)["mean_psnr"]
        model.environment = None
        assert over_zero == evaluate(model, tracer, vb)["mean_psnr"] and with_map != over_zero
