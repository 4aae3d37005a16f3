"""The cube-map background of DESIGN.md §20 without a GPU: the float64 definition is an adjoint pair, the float32 restatement takes
the definition's faces and stays within four times its own measured distance from it, the integer adjoint has its symmetries as
bits, and the host logic — the config block and its refusals, the flags, the checkpoint, the bindings — says what §20 says."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest
import torch

from tests import environment_reference as er
from tests.common import cams, make_view, scenes
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

_capi = importlib.import_module("3dgrut_amd._capi")
environment = importlib.import_module("3dgrut_amd.environment")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
oracle = importlib.import_module("oracle.oracle")

ALL = er.CASES + ("f",)


def _data(name):
    """(rays, M, R, texels [6,R,R,3], cotangent [H,W,3]) of a case: a random map in [0, 1) and a standard-normal cotangent."""
    rays, M, R = er.case(name)
    rng = np.random.default_rng(7 + ord(name))
    return rays, M, R, rng.random((6, R, R, 3)).astype(np.float32), rng.standard_normal(rays.shape).astype(np.float32)


@pytest.mark.parametrize("name", ALL)
def test_the_definition_is_an_adjoint_pair(name):
    """sum_p c . plane(T) = sum_t T . grad(c) in float64, to 1e-9."""
    rays, M, R, T, c = _data(name)
    lhs = float((c.astype(np.float64) * er.sample64(rays, M, T)).sum())
    rhs = float((T.astype(np.float64) * er.adjoint64(rays, M, R, c)).sum())
    assert abs(lhs - rhs) <= 1e-9, (lhs, rhs)


FACES = {"a": 3, "b": 3, "c": 4, "d": 2, "f": 5}      # faces a case reaches, at least


@pytest.mark.parametrize("name", ALL)
def test_the_two_references_take_the_same_faces(name):
    """At least 99.5 % of the pixels (a condition of the comparisons below, asserted so that a later case cannot hide a seam
    behind it); these cases have no disagreement at all."""
    rays, M, R = er.case(name)
    v32, f32, _, _ = er.taps32(rays, M, R)
    v64, f64, _, _ = er.taps64(rays, M, R)
    assert v32.all() and v64.all()
    same = float((f32 == f64).mean())
    print(f"\n[environment {name}] faces {sorted(set(f32.tolist()))} agreement {same}")
    assert same >= 0.995
    assert len(set(f32.tolist())) >= FACES[name]


# The float32 restatement against the float64 definition, measured on _data(name) (max |difference| over the same-face pixels of the
# plane, over the texels of the adjoint).  The texel-coordinate error grows with R and a random map has unit differences between
# neighbours, so the bar is per case: four times the measured value.  The restatement is deterministic; the factor only leaves room
# for another numpy build.
MEASURED_PLANE = {"a": 7.464e-07, "b": 4.417e-05, "c": 9.722e-07, "d": 1.192e-07, "f": 1.254e-06}
MEASURED_ADJOINT = {"a": 5.892e-06, "b": 1.141e-04, "c": 5.003e-06, "d": 1.888e-06, "f": 3.741e-06}


@pytest.mark.parametrize("name", ALL)
def test_the_restatement_stays_near_the_definition(name):
    rays, M, R, T, c = _data(name)
    same = (er.taps32(rays, M, R)[1] == er.taps64(rays, M, R)[1])
    plane = np.abs(er.sample32(rays, M, T).reshape(-1, 3) - er.sample64(rays, M, T).reshape(-1, 3))[same].max()
    adjoint = np.abs(er.adjoint32(rays, M, R, c) - er.adjoint64(rays, M, R, c)).max()
    print(f"\n[environment {name}] restatement - definition: plane {plane:.3e}, adjoint {adjoint:.3e}")
    assert plane <= 4.0 * MEASURED_PLANE[name]
    assert adjoint <= 4.0 * MEASURED_ADJOINT[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ALL)
def test_symmetries_of_the_integer_adjoint(name):
    rays, M, R, _, c = _data(name)
    g = er.adjoint32(rays, M, R, c)
    # (-g written as 0 - g: the exact negation of every non-zero value, and +0 where the sum is zero — the conversion writes
    #  float(0) 2^-s = +0 whatever the sign of c)
    assert np.array_equal(_bits(er.adjoint32(rays, M, R, -c)), _bits(np.float32(0) - g))
    for m in (-20, 3, 60):
        assert np.array_equal(_bits(er.adjoint32(rays, M, R, np.ldexp(c, m))), _bits(np.ldexp(g, m))), m
    holes = c.copy()
    holes[::3, ::5, 0], holes[1::4, ::7, 1], holes[::9, 2::3, 2] = 0.0, 0.0, 0.0
    bad = holes.copy()
    bad[::3, ::5, 0], bad[1::4, ::7, 1], bad[::9, 2::3, 2] = np.nan, np.inf, -np.inf
    assert np.array_equal(_bits(er.adjoint32(rays, M, R, bad)), _bits(er.adjoint32(rays, M, R, holes)))
    zero = er.adjoint32(rays, M, R, np.zeros_like(c))
    assert not _bits(zero).any()                                  # +0 everywhere


def test_the_exponent_function():
    """s = 40 - e with |c| < 2^e, less ceil(log2 P) - 22 beyond 2^22 pixels, clamped to -126 .. 126, 0 for a zero maximum."""
    bits = lambda x: int(np.float32(x).view(np.uint32))
    assert er.scale_exponent(0, 100) == 0
    assert er.scale_exponent(bits(1.0), 100) == 39 and er.scale_exponent(bits(1.5), 100) == 39 and er.scale_exponent(bits(0.99), 100) == 40
    assert er.scale_exponent(bits(2.0 ** 100), 100) == -61
    assert er.scale_exponent(bits(3e38), 100) == -88 and er.scale_exponent(bits(1e-38), 100) == 126      # the clamp
    assert er.scale_exponent(bits(1e-45), 100) == 126                                                      # a denormal maximum
    assert er.scale_exponent(bits(1.0), 1 << 22) == 39 and er.scale_exponent(bits(1.0), (1 << 22) + 1) == 38
    assert er.scale_exponent(bits(1.0), 1 << 30) == 31
    # the sums fit: P products below 2^40 (+ a rounding each) stay below 2^63
    assert (1 << 22) * ((1 << 40) + 4) < (1 << 63)


def test_void_pixels_and_clamping():
    """Zero and non-finite directions are void (+0, nothing scattered); at R = 1 every index clamps to the one texel of the face, so
    the plane IS that texel where the weights sum to 1."""
    rays, M, R = er.case("d")
    rays = rays.copy()
    rays[0, 0], rays[1, 1, 2], rays[2, 2, 0] = 0.0, np.nan, np.inf
    T = np.random.default_rng(0).random((6, 1, 1, 3)).astype(np.float32)
    valid, face, texel, w = er.taps32(rays, M, 1)
    assert (~valid).sum() == 3
    plane = er.sample32(rays, M, T).reshape(-1, 3)
    assert not _bits(plane[~valid]).any()
    assert np.array_equal(texel[valid], np.repeat(face[valid, None], 4, axis=1))
    assert np.abs(plane[valid] - T.reshape(6, 3)[face[valid]]).max() <= 2e-7
    c = np.ones(rays.shape, np.float32)
    g = er.adjoint64(rays, M, 1, c)
    assert abs(g.sum() - 3.0 * valid.sum()) <= 1e-6


# ---- host logic ----
def test_config_rules():
    blk = trainer_mod.resolve_config({})["environment"]
    assert blk == {"enabled": False, "resolution": 256, "lr": 0.01, "init": 0.5, "start_iteration": 0, "end_iteration": None}
    assert trainer_mod.resolve_config({})["model"]["background"] == {"name": "background-color", "color": "black"}
    ok = trainer_mod.resolve_config({"environment": {"enabled": True, "resolution": 16, "lr": 0.0, "init": -1.5, "start_iteration": 3, "end_iteration": 9}})
    assert ok["environment"]["enabled"] is True and ok["environment"]["end_iteration"] == 9
    for override, words in (({"resolution": 0}, "environment.resolution must be an integer in 1 .. 8192, got 0"),
                            ({"resolution": 8193}, "environment.resolution must be an integer in 1 .. 8192, got 8193"),
                            ({"resolution": 16.0}, "environment.resolution must be an integer in 1 .. 8192, got 16.0"),
                            ({"lr": -0.1}, "environment.lr must be finite and >= 0, got -0.1"),
                            ({"lr": "0.1"}, "environment.lr must be finite and >= 0, got '0.1'"),
                            ({"init": float("nan")}, "environment.init must be finite, got nan"),
                            ({"enabled": 1}, "environment.enabled must be true or false, got 1"),
                            ({"start_iteration": -1}, "environment.start_iteration must be an integer >= 0, got -1"),
                            ({"end_iteration": -1}, "environment.end_iteration must be null or an integer >= 0, got -1"),
                            ({"colour": 1}, "environment: unknown keys ['colour']")):
        with pytest.raises(ValueError) as e:
            trainer_mod.resolve_config({"environment": override})
        assert str(e.value) == words


def test_the_three_refusals():
    for color in ("white", "random"):
        with pytest.raises(ValueError, match="environment: the map is the background, model.background.color must be 'black'"):
            trainer_mod.resolve_config({"environment": {"enabled": True}, "model": {"background": {"color": color}}})
        assert trainer_mod.resolve_config({"model": {"background": {"color": color}}})["environment"]["enabled"] is False
    with pytest.raises(ValueError, match="environment: pose-aligned metrics are refused with an environment map"):
        trainer_mod.resolve_config({"environment": {"enabled": True}, "pose_alignment": {"enabled": True}})
    st = _FakeStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError) as e:
        _trainer({"n_iterations": 1, "environment": {"enabled": True, "resolution": 4}}, stepper=st)
    assert str(e.value) == "environment: data-parallel environment-map training is out of scope (the stepper's world_size must be 1)"
    assert trainer_mod.resolve_config({"environment": {"enabled": True}, "pose_refinement": {"enabled": True}})["environment"]["enabled"]   # composes


def test_flags():
    """The three flags are a table of their own, parsed by main() behind the recorded ones: the default parser and the conf of a
    command line without them are what they were."""
    flags = trainer_mod.FLAGS + trainer_mod.ENVIRONMENT_FLAGS
    parser = trainer_mod.build_parser(flags)
    conf_of = lambda argv: trainer_mod.config_from_args(parser.parse_args(["--path", "scene"] + argv), flags)
    assert conf_of([])["environment"] == {"enabled": False}
    assert trainer_mod.resolve_config(conf_of([]))["environment"] == environment.DEFAULTS
    assert trainer_mod.resolve_config(conf_of(["--environment"]))["environment"] == dict(environment.DEFAULTS, enabled=True)
    got = trainer_mod.resolve_config(conf_of(["--environment", "--environment-resolution", "64", "--environment-lr", "0.002"]))["environment"]
    assert got == dict(environment.DEFAULTS, enabled=True, resolution=64, lr=0.002)
    assert [f for f, _, _, _ in trainer_mod.ENVIRONMENT_FLAGS] == ["--environment", "--environment-resolution", "--environment-lr"]
    assert "environment" not in trainer_mod.config_from_args(trainer_mod.build_parser().parse_args(["--path", "scene"]))
    assert "environment" not in trainer_mod.default_config()
    with pytest.raises(SystemExit):
        trainer_mod.build_parser().parse_args(["--path", "scene", "--environment"])
    assert "--environment [--environment-resolution R] [--environment-lr X]" in trainer_mod.__doc__


def test_checkpoint_keys_resume_and_the_resume_refusal(tmp_path):
    tr, st, _, _, _ = _trainer({"n_iterations": 2, "environment": {"enabled": True, "resolution": 4, "init": 0.25, "end_iteration": 1}})
    env = tr.environment_map
    assert tr.model.environment is env and tuple(env.texels.shape) == (6, 4, 4, 3) and float(env.texels[0, 0, 0, 0]) == 0.25
    assert [env.active(g) for g in range(3)] == [True, False, False]
    tr.train()
    assert st.environment_active is False                    # the window's switch of the last step
    assert tr.stats["environment_resolution"] == 4 and tr.stats["environment_mean_colour"] == [0.25, 0.25, 0.25]
    assert torch.equal(tr.environment(), torch.full((6, 4, 4, 3), 0.25))
    # a state to carry: one Adam step from a gradient of ones
    env.texels.grad = torch.ones_like(env.texels)
    env.step()
    ckpt = tr.checkpoint()
    saved = ckpt["native"]["environment"]
    assert set(saved) == {"texels", "exp_avg", "exp_avg_sq", "step"} and all(isinstance(v, torch.Tensor) for v in saved.values())
    assert float(saved["step"]) == 1.0 and torch.equal(saved["texels"], env.texels)
    path = str(tmp_path / "ckpt.pt")
    torch.save(ckpt, path)
    assert set(torch.load(path, map_location="cpu", weights_only=True)["native"]["environment"]) == set(saved)
    # resumed: the same texels and Adam state, and the next step lands on the same bits
    tr2, _, _, _, _ = _trainer({"n_iterations": 2, "resume": path, "environment": {"enabled": True, "resolution": 4, "init": 0.9}},
                               stepper=_FakeStepper(_model()))
    env2 = tr2.environment_map
    assert torch.equal(env2.texels, env.texels)
    for e in (env, env2):
        e.texels.grad = torch.full_like(e.texels, 0.5)
        e.step()
    assert torch.equal(env2.texels, env.texels) and not torch.equal(env.texels, saved["texels"])
    with pytest.raises(ValueError, match="the checkpoint holds a map of resolution 4, this run has 8"):
        _trainer({"n_iterations": 2, "resume": path, "environment": {"enabled": True, "resolution": 8}}, stepper=_FakeStepper(_model()))
    with pytest.raises(ValueError, match="environment: the checkpoint holds an environment map and environment.enabled is off; resume with --environment"):
        _trainer({"n_iterations": 2, "resume": path}, stepper=_FakeStepper(_model()))
    # without a map: no key, no attribute set
    tr3, _, _, _, _ = _trainer({"n_iterations": 1})
    assert "environment" not in tr3.checkpoint()["native"] and tr3.environment_map is None and tr3.environment() is None
    assert tr3.model.environment is None


def test_bindings():
    lib = _capi.load()
    assert lib.gut_abi_version() == 6 == _capi.GUT_ABI_VERSION
    for name in ("gut_environment_sample", "gut_environment_workspace_bytes", "gut_environment_backward", "gut_environment_rotation"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.gut_environment_sample.argtypes == [vp, C.POINTER(_capi.GutEnvironmentView), vp, i32, vp]
    assert lib.gut_environment_backward.argtypes == [vp, C.POINTER(_capi.GutEnvironmentView), C.POINTER(_capi.GutEnvironmentCotangent), i32, vp, vp]
    assert lib.gut_environment_workspace_bytes.argtypes == [i32] and lib.gut_environment_workspace_bytes.restype is C.c_size_t
    assert C.sizeof(_capi.GutEnvironmentView) == 56 and C.sizeof(_capi.GutEnvironmentCotangent) == 24
    assert _capi.kEnvSlots == 128 and _capi.ENVIRONMENT_TILE == er.TILE
    assert lib.gut_environment_workspace_bytes(16) == 8 * 18 * 16 * 16 + 16
    assert lib.gut_environment_workspace_bytes(0) == 0 and lib.gut_environment_workspace_bytes(_capi.ENVIRONMENT_MAX_RESOLUTION + 1) == 0
    assert 18 * _capi.ENVIRONMENT_MAX_RESOLUTION ** 2 < 2 ** 31
    # the header says what the bindings say
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gut_hip.h")).read()
    assert "#define GUT_ENVIRONMENT_SLOTS 128" in header and "#define GUT_ENVIRONMENT_MAX_RESOLUTION 8192" in header
    assert "#define GUT_ABI_VERSION 6" in header


def test_error_returns_are_host_side():
    """Every refusal is decided before anything is queued, so it is the same without a GPU: nothing here launches."""
    lib = _capi.load()
    rays = np.zeros((4, 4, 3), np.float32)
    some = rays.ctypes.data          # never dereferenced: every call below is refused on the host
    view = lambda ptr=some, h=4, w=4: _capi.GutEnvironmentView(ptr, (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), h, w)
    plane = _capi.GutEnvironmentCotangent(some, None, None)

    def refused(rc, words):
        assert rc != 0 and words in lib.gut_last_error().decode(), lib.gut_last_error()
    refused(lib.gut_environment_sample(None, None, some, 4, some), "null view")
    refused(lib.gut_environment_sample(None, C.byref(view(None)), some, 4, some), "null d_ray_direction")
    refused(lib.gut_environment_sample(None, C.byref(view()), None, 4, some), "null d_texels or d_plane_out")
    refused(lib.gut_environment_sample(None, C.byref(view()), some, 4, None), "null d_texels or d_plane_out")
    refused(lib.gut_environment_sample(None, C.byref(view()), some, 0, some), "resolution must be 1 .. 8192, got 0")
    refused(lib.gut_environment_sample(None, C.byref(view()), some, 8193, some), "resolution must be 1 .. 8192, got 8193")
    refused(lib.gut_environment_sample(None, C.byref(view(h=0)), some, 4, some), "an empty image")
    refused(lib.gut_environment_backward(None, C.byref(view(w=0)), C.byref(plane), 4, some, some), "an empty image")
    refused(lib.gut_environment_backward(None, C.byref(view()), None, 4, some, some), "null cotangent")
    refused(lib.gut_environment_backward(None, C.byref(view()), C.byref(plane), 4, None, some), "null d_workspace or d_texel_grad")
    refused(lib.gut_environment_backward(None, C.byref(view()), C.byref(plane), 4, some, None), "null d_workspace or d_texel_grad")
    refused(lib.gut_environment_backward(None, C.byref(view()), C.byref(plane), -3, some, some), "resolution must be 1 .. 8192, got -3")
    for cot in (_capi.GutEnvironmentCotangent(None, None, None), _capi.GutEnvironmentCotangent(None, some, None),
                _capi.GutEnvironmentCotangent(some, some, some), _capi.GutEnvironmentCotangent(some, None, some)):
        refused(lib.gut_environment_backward(None, C.byref(view()), C.byref(cot), 4, some, some), "either d_plane_grad or the pair")


def test_the_rotation_is_the_compositors():
    """rotation_from_pose gives the camera-to-world rotation the rays are turned by: the oracle's sensor-to-world matrix to a few
    float32 roundings (the oracle round-trips it through a quaternion), the float64 pose to the same."""
    for c2w in (cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)), cams.orbit_c2w(4.0, 135.0, 20.0)):
        view = make_view("pinhole", 32, 32, c2w)
        M = environment.rotation_from_pose(torch.as_tensor(view["c2w"])[None]).reshape(3, 3)
        assert M.dtype == np.float32
        s2w = oracle.pose_matrices(dict(view["oracle_cam"], pose_end=view["tq"]))[2]
        assert np.abs(M - s2w[:, :3]).max() <= 1e-6
        assert np.abs(M.astype(np.float64) - np.asarray(c2w, np.float64)[:3, :3]).max() <= 1e-6
    sig = inspect.signature(environment.EnvironmentMap.__init__)
    assert list(sig.parameters)[1:4] == ["resolution", "init", "device"] and sig.parameters["init"].default == 0.5


# ---- the recovery test's precondition ----
RECOVERY_R = 16


def recovery_views():
    """The eight orbit views at 128 x 128 of tests/test_gpu_pose_gradient.py."""
    return [make_view("pinhole", 128, 128, cams.orbit_c2w(4.0, 360.0 * i / 8, 10.0 + 20.0 * (i % 3) / 2.0)) for i in range(8)]


def recovery_coverage(alphas, views=None):
    """sum_p (1 - alpha) w per texel of the R = 16 map over the views, float64 [6,16,16]."""
    cover = np.zeros((6, RECOVERY_R, RECOVERY_R, 3))
    for view, alpha in zip(views or recovery_views(), alphas):
        M = environment.rotation_from_pose(view["c2w"])
        c = np.repeat(1.0 - np.asarray(alpha, np.float64).reshape(128, 128, 1), 3, axis=2)
        cover += er.adjoint64(view["rd"].reshape(128, 128, 3), M.reshape(3, 3), RECOVERY_R, c)
    return cover[..., 0]


def test_the_recovery_test_has_texels_to_recover():
    """With the oracle's alpha for the eight views of the GPU recovery test, at least 100 texels receive sum_p (1 - alpha) w >= 1."""
    sc = scenes.scene_c1(1000, 0)
    act = np.zeros((1000, 12), np.float32)
    act[:, 0:3], act[:, 3:4], act[:, 4:8], act[:, 8:11] = sc["positions"], sc["density"], sc["rotation"], sc["scale"]
    alphas = []
    for view in recovery_views():
        fwd = oracle.forward(dict(view["oracle_cam"], pose_end=view["tq"]), 128, 128, act, sc["features"], view["ro"], view["rd"])
        alphas.append(fwd["rgba"][..., 3])
    cover = recovery_coverage(alphas)
    n = int((cover >= 1.0).sum())
    print(f"\n[environment recovery] texels with coverage >= 1: {n} of {cover.size}, open share {1.0 - float(np.mean(alphas)):.3f}")
    assert n >= 100


def test_to_equirect():
    """A lat-long image of the map in torch: a constant map gives that constant; with one colour per face the top row is +y (face 2),
    the bottom row -y (face 3), and the middle row runs +z, -x, -z, +x, +z from left to right."""
    env = environment.EnvironmentMap(4, 0.25, "cpu")
    img = env.to_equirect(16)
    assert tuple(img.shape) == (16, 32, 3) and float((img - 0.25).abs().max()) <= 1e-6
    for face in range(6):
        env.texels[face] = float(face)
    img = env.to_equirect(16)[..., 0]
    assert float((img[0] - 2.0).abs().max()) <= 1e-6 and float((img[-1] - 3.0).abs().max()) <= 1e-6
    mid = img[8]
    assert [round(float(mid[c])) for c in (0, 8, 16, 24, 31)] == [4, 1, 5, 0, 4]
