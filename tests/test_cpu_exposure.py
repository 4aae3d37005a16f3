"""Per-view exposure compensation without a GPU: the torch definition of the affine image and its gradient, the per-view Adam
bookkeeping of ExposureCompensation on host tensors, its place in the Trainer (with the fake stepper of tests/test_cpu_trainer.py,
as tests/test_cpu_pose_refiner.py uses it), the checkpoint round trip, the config validation and the C ABI surface."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests.test_cpu_pose_refiner import _views
from tests.test_cpu_trainer import _FakeEvaluator, _FakeStepper, _FakeStrategy, _model

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
native = importlib.import_module("3dgrut_amd.native")
losses = importlib.import_module("3dgrut_amd.losses")
exposure = importlib.import_module("3dgrut_amd.exposure")
capi = importlib.import_module("3dgrut_amd._capi")

E_TEST = torch.tensor([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.03], [0.02, -0.05, 1.20, 0.04]], dtype=torch.float64)
IDENTITY = torch.tensor(exposure.IDENTITY)


# ---- the definition ----
def _images(H=14, W=15, seed=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((1, H, W, 3), generator=g, dtype=torch.float64), torch.rand((1, H, W, 3), generator=g, dtype=torch.float64),
            (torch.rand((1, H, W, 1), generator=g) > 0.2).double())


@pytest.mark.parametrize("masked", [False, True])
def test_exposure_gradient_of_the_torch_definition_against_finite_differences(masked):
    """fp64 autograd dE of losses.photometric_loss(..., exposure=E) on a 14 x 15 image against central differences of step 1e-6:
    truncation ~ h^2 and rounding ~ 1e-16 / h are both far below the 1e-6 rel-L2 bound (|x| kinks of the L1 term within h of a
    pixel difference of zero would break it: the random images have none that close)."""
    pred, gt, mask = _images()
    mask = mask if masked else None
    E = E_TEST.clone().requires_grad_(True)
    loss = losses.photometric_loss(pred, gt, 0.8, 0.2, mask=mask, exposure=E)
    loss.backward()
    h, fd = 1e-6, torch.zeros(12, dtype=torch.float64)
    with torch.no_grad():
        for k in range(12):
            d = torch.zeros(12, dtype=torch.float64)
            d[k] = h
            up = losses.photometric_loss(pred, gt, 0.8, 0.2, mask=mask, exposure=(E_TEST.reshape(12) + d))
            dn = losses.photometric_loss(pred, gt, 0.8, 0.2, mask=mask, exposure=(E_TEST.reshape(12) - d).reshape(3, 4))
            fd[k] = (up - dn) / (2 * h)
    err = float((E.grad.reshape(12) - fd).norm() / fd.norm())
    print(f"\n[exposure definition masked={masked}] dE rel-L2 against central differences {err:.3e}")
    assert float(fd.abs().min()) > 0 and err <= 1e-6, err


def test_identity_exposure_is_the_plain_loss():
    pred, gt, mask = _images()
    for m in (None, mask):
        plain = losses.photometric_loss(pred, gt, 0.8, 0.2, mask=m)
        same = losses.photometric_loss(pred, gt, 0.8, 0.2, mask=m, exposure=IDENTITY.double())
        assert float(plain) == float(same)
        assert float(losses.photometric_loss(pred, gt, 0.8, 0.2, mask=m, exposure=E_TEST)) != float(plain)
    out = losses.apply_exposure(pred, E_TEST)
    px = pred[0, 3, 4]
    assert torch.allclose(out[0, 3, 4], E_TEST[:, :3] @ px + E_TEST[:, 3], rtol=1e-14, atol=0)


# ---- the per-view state ----
def _grad12(seed):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal(12), dtype=torch.float32)


def test_only_the_visited_views_row_moments_and_count_move():
    ex = exposure.ExposureCompensation(3, "cpu", lr=1e-3)
    assert tuple(ex.params.shape) == (3, 12) and all(torch.equal(ex.params[v], IDENTITY) for v in range(3))
    views = _views(3)
    g = _grad12(0)
    out = ex.begin(1, views[1])
    assert out is not views[1] and out.tag == 1 and not hasattr(views[1], "exposure")          # the caller's batch is untouched
    assert out.exposure.data_ptr() == ex.params[1].data_ptr() and tuple(out.exposure.shape) == (12,)   # a view, not a copy
    ex.end(1, g)
    assert ex.counts.tolist() == [0, 1, 0]
    for v in (0, 2):
        assert torch.equal(ex.params[v], IDENTITY) and not ex.m[v].any() and not ex.v[v].any()
    # Adam's first step from zero moments: m = (1 - b1) g, v = (1 - b2) g^2, bias-corrected by the view's OWN count (1): the entry
    # moves by -lr * sign(g) up to eps
    assert torch.allclose(ex.m[1], 0.1 * g, rtol=1e-6, atol=0)
    assert torch.allclose(ex.v[1], 0.001 * g ** 2, rtol=1e-4, atol=0)   # (1 - beta2 is held in float32: 0.0010000467)
    assert torch.allclose(ex.params[1] - IDENTITY, -1e-3 * torch.sign(g), rtol=1e-3, atol=0)   # (the difference of two floats near 1)
    assert torch.equal(out.exposure, ex.params[1])                       # the handed-out row IS the state
    # another view starts its own count at 1: the same first step
    ex.end(2, g)
    assert ex.counts.tolist() == [0, 1, 1] and torch.equal(ex.params[2], ex.params[1]) and torch.equal(ex.m[2], ex.m[1])
    # the second visit of view 1 uses count 2
    ex.end(1, g)
    assert ex.counts.tolist() == [0, 2, 1]
    m2 = 0.9 * (0.1 * g) + 0.1 * g
    v2 = 0.999 * (0.001 * g ** 2) + 0.001 * g ** 2
    assert torch.allclose(ex.m[1], m2, rtol=1e-5, atol=0)
    step2 = -1e-3 * (m2 / (1 - 0.9 ** 2)) / (v2 / (1 - 0.999 ** 2)).sqrt()
    assert torch.allclose(ex.params[1] - ex.params[2], step2, rtol=2e-3, atol=0)
    with pytest.raises(ValueError, match="the gradient is on"):
        ex.end(0, torch.zeros(12, device="meta"))
    with pytest.raises(ValueError, match="12 float32"):
        ex.end(0, torch.zeros(8))
    E = ex.exposures()
    assert tuple(E.shape) == (3, 3, 4) and torch.equal(E[0], IDENTITY.reshape(3, 4))
    s = ex.summary()
    assert s["mean_gain"] == pytest.approx(float(torch.diagonal(E[:, :, :3], dim1=1, dim2=2).mean()))
    assert s["mean_offset"] == pytest.approx(float(E[:, :, 3].abs().mean())) and s["mean_offset"] > 0


def test_window_of_iterations():
    ex = exposure.ExposureCompensation(2, "cpu", start_iteration=5, end_iteration=9)
    assert [g for g in range(12) if ex.active(g)] == [5, 6, 7, 8]
    ex = exposure.ExposureCompensation(2, "cpu", start_iteration=2)
    assert not ex.active(1) and ex.active(2) and ex.active(10 ** 9)
    assert not any(exposure.ExposureCompensation(2, "cpu", end_iteration=0).active(g) for g in range(5))


def test_state_dict_round_trips_bit_for_bit(tmp_path):
    ex = exposure.ExposureCompensation(3, "cpu", lr=2e-3)
    for k, v in enumerate((0, 2, 2, 1, 2)):
        ex.end(v, _grad12(k))
    path = tmp_path / "exposure.pt"
    torch.save(dict(native=dict(exposure=ex.state_dict())), path)
    saved = torch.load(path, weights_only=True)["native"]["exposure"]
    assert all(isinstance(x, torch.Tensor) for x in saved.values())
    other = exposure.ExposureCompensation(3, "cpu", lr=2e-3)
    row = other.params[2]
    other.load_state_dict(saved)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(other.params), bits(ex.params)) and torch.equal(bits(other.m), bits(ex.m))
    assert torch.equal(bits(other.v), bits(ex.v)) and torch.equal(other.counts, ex.counts) and ex.counts.tolist() == [1, 1, 3]
    assert torch.equal(row, ex.params[2])                      # loaded in place: rows handed out before stay views of the state
    ex.end(2, _grad12(9))
    other.end(2, _grad12(9))
    assert torch.equal(bits(other.params), bits(ex.params))
    with pytest.raises(ValueError, match="training views"):
        exposure.ExposureCompensation(4, "cpu").load_state_dict(saved)


# ---- the trainer ----
class _ExposureStepper(_FakeStepper):
    """The fake stepper with NativeTrainStep(exposure_gradient=True)'s surface: step() leaves a gradient that depends on the view."""
    world_size = 1

    def __init__(self, model, seed=0):
        super().__init__(model, seed)
        self._buffer = torch.zeros(12)
        self.exposure_gradient = self._buffer
        self.seen = []
        self.switched = []

    def enable_exposure_gradient(self, on):
        self.switched.append(bool(on))

    def step(self, batch):
        self.seen.append((batch.tag, batch.exposure.clone(), batch.exposure.data_ptr()))
        self._buffer.copy_(_grad12(100 + batch.tag))
        return super().step(batch)


def _trainer(conf, views=3, stepper=None):
    conf = dict(conf, strategy=dict(method="GSStrategy"))
    st = stepper or _ExposureStepper(_model())
    return trainer_mod.Trainer(conf, None, _views(views), val_batches=_views(1), scene_extent=2.0, stepper=st, strategy=_FakeStrategy(),
                               evaluator=_FakeEvaluator()), st


def test_option_is_off_by_default_and_validated():
    conf = trainer_mod.resolve_config({})
    assert conf["exposure"] == exposure.DEFAULTS and conf["exposure"]["enabled"] is False
    assert exposure.DEFAULTS == dict(enabled=False, lr=0.001, start_iteration=0, end_iteration=-1, beta1=0.9, beta2=0.999, eps=1e-15)
    tr, st = _trainer(dict(n_iterations=4, val_frequency=1000), stepper=_FakeStepper(_model()))
    assert tr.exposure is None
    tr.train()
    assert torch.equal(tr.exposures(), IDENTITY.reshape(1, 3, 4).repeat(3, 1, 1)) and "exposure_mean_gain" not in tr.stats
    assert "exposure" not in tr.checkpoint()["native"]
    with pytest.raises(ValueError, match="beta1"):
        trainer_mod.resolve_config(dict(exposure=dict(beta1=1.0)))
    with pytest.raises(ValueError, match="beta2"):
        trainer_mod.resolve_config(dict(exposure=dict(beta2=-0.1)))
    with pytest.raises(ValueError, match="lr"):
        trainer_mod.resolve_config(dict(exposure=dict(lr=-1.0)))
    with pytest.raises(ValueError, match="unknown"):
        trainer_mod.resolve_config(dict(exposure=dict(learning_rate=1.0)))
    with pytest.raises(ValueError, match="enabled"):
        trainer_mod.resolve_config(dict(exposure=dict(enabled="false")))
    for bad in (dict(start_iteration=1.5), dict(end_iteration="10"), dict(start_iteration=-1), dict(end_iteration=-2), dict(start_iteration=True)):
        with pytest.raises(ValueError, match="iteration"):
            trainer_mod.resolve_config(dict(exposure=bad))
    # a stepper that leaves no exposure gradient cannot learn exposures; nor can a data-parallel one
    with pytest.raises(ValueError, match="exposure gradient"):
        _trainer(dict(exposure=dict(enabled=True)), stepper=_FakeStepper(_model()))
    dp = _ExposureStepper(_model())
    dp.world_size = 2
    with pytest.raises(ValueError, match="world_size"):
        _trainer(dict(exposure=dict(enabled=True)), stepper=dp)
    with pytest.raises(ValueError, match="world_size"):
        native.NativeTrainStep(None, None, world_size=2, exposure_gradient=True)


def test_command_line_switches_fill_the_block():
    ap = trainer_mod.build_parser()
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--exposure", "--exposure-lr", "0.002"]))
    assert conf["exposure"] == dict(exposure.DEFAULTS, enabled=True, lr=0.002)
    assert conf["pose_refinement"]["enabled"] is False                  # independent of --refine-poses
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert conf["exposure"] == exposure.DEFAULTS
    trainer_mod.resolve_config(conf)


def test_trainer_loop_hands_every_view_its_own_row_and_resumes_bit_for_bit(tmp_path):
    conf = dict(n_iterations=7, val_frequency=1000, exposure=dict(enabled=True, lr=2e-3, start_iteration=1))
    tr, st = _trainer(conf)
    assert tr.exposure.lr == pytest.approx(2e-3) and tr.exposure.num_views == 3
    tr.train()
    assert st.switched == [False] + [True] * 6                    # the reduction is off outside [start_iteration, end_iteration)
    order = [v for v, _, _ in st.seen]
    assert order == [tr.batch_index(g) for g in range(7)]
    visits = {v: sum(1 for g, w in enumerate(order) if w == v and g >= 1) for v in range(3)}
    assert tr.exposure.counts.tolist() == [visits[v] for v in range(3)]
    # every step saw the row of its own view (a view of the state), holding the updates of that view's EARLIER visits only
    replay = exposure.ExposureCompensation(3, "cpu", lr=2e-3, start_iteration=1)
    for g, (v, E, ptr) in enumerate(st.seen):
        assert ptr == tr.exposure.params[v].data_ptr(), (g, v)
        assert torch.equal(E, replay.params[v]), (g, v)
        if replay.active(g):
            replay.end(v, _grad12(100 + v))
    assert torch.equal(tr.exposure.params, replay.params)
    assert any(not torch.equal(E, IDENTITY) for _, E, _ in st.seen)
    assert all(not hasattr(b, "exposure") for b in tr.train_batches)          # the caller's batches stay untouched
    E = tr.exposures()
    assert E.dtype == torch.float32 and tuple(E.shape) == (3, 3, 4) and torch.equal(E.reshape(3, 12), tr.exposure.params)
    assert tr.stats["exposure_mean_gain"] == pytest.approx(float(torch.diagonal(E[:, :, :3], dim1=1, dim2=2).mean()))
    assert tr.stats["exposure_mean_offset"] == pytest.approx(float(E[:, :, 3].abs().mean())) and tr.stats["exposure_mean_offset"] > 0

    ck = tr.checkpoint()
    path = tmp_path / "ckpt.pt"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=True)            # tensors only under `native`
    saved = ck["native"]["exposure"]
    assert all(isinstance(x, torch.Tensor) for x in saved.values()) and "pose_refinement" not in ck["native"]
    with pytest.raises(ValueError, match="end_iteration 0"):      # a resume must not silently drop the learnt exposures
        _trainer(dict(n_iterations=9, val_frequency=1000, resume=str(path)))
    tr2, st2 = _trainer(dict(conf, n_iterations=9, resume=str(path)))
    assert tr2.global_step == 7
    assert torch.equal(tr2.exposure.params, tr.exposure.params) and torch.equal(tr2.exposure.m, tr.exposure.m)
    assert torch.equal(tr2.exposure.v, tr.exposure.v) and torch.equal(tr2.exposure.counts, tr.exposure.counts)
    # the resumed run continues as the uninterrupted one would
    tr3, st3 = _trainer(dict(conf, n_iterations=9))
    tr3.train()
    tr2.train()
    assert [v for v, _, _ in st2.seen] == [v for v, _, _ in st3.seen][7:]
    for (_, a, _), (_, b, _) in zip(st2.seen, st3.seen[7:]):
        assert torch.equal(a, b)
    assert torch.equal(tr2.exposures(), tr3.exposures())
    # frozen: end_iteration 0 keeps the saved exposures as they are, and still hands them to every step
    tr4, st4 = _trainer(dict(n_iterations=9, val_frequency=1000, resume=str(path), exposure=dict(enabled=True, end_iteration=0)))
    tr4.train()
    assert st4.switched == [False, False] and torch.equal(tr4.exposure.params, tr.exposure.params)
    assert all(torch.equal(E, tr.exposure.params[v]) for v, E, _ in st4.seen)


def test_exposure_composes_with_pose_refinement():
    """Both options on: the step sees the refined pose AND the view's exposure row; each state advances on its own."""
    from tests.test_cpu_pose_refiner import _grad8

    class Both(_ExposureStepper):
        def __init__(self, model):
            super().__init__(model)
            self.pose_gradient = torch.zeros(8)

        def step(self, batch):
            self.pose_gradient.copy_(_grad8(batch.tag))
            assert tuple(batch.T_to_world.shape) == (1, 4, 4)
            return super().step(batch)

    tr, st = _trainer(dict(n_iterations=6, val_frequency=1000, exposure=dict(enabled=True), pose_refinement=dict(enabled=True)),
                      stepper=Both(_model()))
    tr.train()
    assert tr.exposure.counts.tolist() == [2, 2, 2] and tr.refiner.counts.tolist() == [2, 2, 2]
    nat = tr.checkpoint()["native"]
    assert "exposure" in nat and "pose_refinement" in nat


# ---- the C ABI ----
def test_new_symbols_are_exported_and_declared():
    lib = capi.load()
    names = ("gut_photometric_exposure_workspace_bytes", "gut_photometric_loss_exposure", "gut_exposure_adam_step")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.gut_photometric_exposure_workspace_bytes.restype is C.c_size_t
    assert len(lib.gut_photometric_loss_exposure.argtypes) == 15 and len(lib.gut_exposure_adam_step.argtypes) == 10
    assert lib.gut_abi_version() == 6 == capi.GUT_ABI_VERSION
    for hw in ((37, 53), (1237, 822)):
        # its own size function: the existing one keeps its value, the new form needs room for the rows of 12 partials
        assert lib.gut_photometric_exposure_workspace_bytes(*hw) >= lib.gut_photometric_workspace_bytes(*hw) + 12 * 4
    # null pointers and small images are refused before anything is launched (no GPU needed for that)
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert lib.gut_photometric_loss_exposure(None, 37, 53, p, p, None, None, 0.0, None, 0.8, 0.2, p, p, p, None) == 1
    assert lib.gut_photometric_loss_exposure(None, 10, 53, p, p, None, None, 0.0, p, 0.8, 0.2, p, p, p, None) == 1
    assert lib.gut_exposure_adam_step(None, p, p, p, None, p, 1e-3, 0.9, 0.999, 1e-15) == 1
