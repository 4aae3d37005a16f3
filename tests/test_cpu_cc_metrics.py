"""Colour-corrected held-out metrics without a GPU: the C ABI surface and its host-side refusals, the float64 torch
restatement losses.colour_correction against an augmented least-squares solve (tests/cc_reference.py: a different algorithm from
the normal equations), the two exact properties of the ridge, and the option's path through the Trainer with a fake evaluator in
the style of tests/test_cpu_exposure.py."""
import ctypes as C
import importlib
import json

import numpy as np
import pytest
import torch

from tests import cc_reference as ref
from tests.test_cpu_exposure import _ExposureStepper
from tests.test_cpu_pose_refiner import _views
from tests.test_cpu_trainer import _FakeStepper, _FakeStrategy, _model

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
losses = importlib.import_module("3dgrut_amd.losses")
capi = importlib.import_module("3dgrut_amd._capi")

CASES = [(hw, kind, bg) for hw in ref.SHAPES for kind in ref.KINDS for bg in ref.BACKGROUNDS]


# ---- the C ABI ----
def test_new_symbols_are_exported_and_declared():
    lib = capi.load()
    for name in ("gut_image_metrics_cc_workspace_bytes", "gut_image_metrics_cc"):
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.gut_image_metrics_cc_workspace_bytes.restype is C.c_size_t and len(lib.gut_image_metrics_cc_workspace_bytes.argtypes) == 2
    assert len(lib.gut_image_metrics_cc.argtypes) == 10
    assert lib.gut_abi_version() == 6 == capi.GUT_ABI_VERSION
    for H, W in ref.SHAPES + [(1237, 822)]:
        rows = -(-H * W // 1024)
        # the metrics' partials, one row of 22 doubles per 1024 pixels, the fitted E
        assert lib.gut_image_metrics_cc_workspace_bytes(H, W) >= lib.gut_image_metrics_workspace_bytes(H, W) + rows * 22 * 8 + 48
        assert len(capi.EXPORTS) == len(set(capi.EXPORTS))


def test_refusals_run_on_the_host_before_anything_is_queued():
    """Null pointers, a 10-pixel side and a ridge that is 0, negative, NaN or infinite return 1 on a machine without a GPU."""
    lib = capi.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    call = lambda H, W, rgba, gt, ridge, ws, out, E=None: lib.gut_image_metrics_cc(None, H, W, rgba, gt, 0.0, ridge, ws, out, E)
    assert call(37, 53, None, p, 1e-6, p, p) == 1
    assert call(37, 53, p, None, 1e-6, p, p) == 1
    assert call(37, 53, p, p, 1e-6, None, p) == 1
    assert call(37, 53, p, p, 1e-6, p, None, p) == 1
    assert call(10, 53, p, p, 1e-6, p, p) == 1 and call(53, 10, p, p, 1e-6, p, p, p) == 1
    for ridge in (0.0, -1e-6, float("nan"), float("inf")):
        assert call(37, 53, p, p, ridge, p, p) == 1, ridge
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ridge"):
            losses.colour_correction(torch.rand(4, 4, 3), torch.rand(4, 4, 3), ridge=bad)
        with pytest.raises(ValueError, match="ridge"):
            losses.image_metrics_colour_corrected(torch.rand(12, 12, 4), torch.rand(12, 12, 3), ridge=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.image_metrics_colour_corrected(torch.rand(12, 12, 4), torch.rand(12, 12, 3))
    with pytest.raises(ValueError, match="background"):
        losses.image_metrics_colour_corrected(torch.rand(12, 12, 4), torch.rand(12, 12, 3), background="grey")


# ---- the definition ----
@pytest.mark.parametrize("hw,kind,background", CASES)
def test_colour_correction_matches_the_augmented_least_squares_fit(hw, kind, background):
    """losses.colour_correction (normal equations, Cholesky) against lstsq on the stacked rows: 1e-9 per entry.  With cond(G) <= 1e4
    (asserted on the reference) double normal equations lose about cond * 1e-16 = 1e-12.  And SSE(E) <= SSE(I), exactly: the
    objective at E is at most the objective at the identity, whose ridge term is zero."""
    rgba, gt = ref.images(*hw, kind, background)
    comp = ref.composite(rgba, background)
    E_ref, cond = ref.reference_fit(comp, gt)
    assert cond <= 1e4, cond
    E = losses.colour_correction(comp, gt, ridge=ref.RIDGE)
    assert E.dtype == torch.float64 and tuple(E.shape) == (3, 4)
    err = float(np.abs(E.numpy() - E_ref).max())
    assert err <= 1e-9, err
    assert ref.sse(comp, gt, E) <= ref.sse(comp, gt, ref.IDENTITY34)
    assert ref.sse(comp, gt, E_ref) <= ref.sse(comp, gt, ref.IDENTITY34)


def test_degenerate_images_stay_finite():
    """A constant-colour image leaves G singular without the ridge; with it E is finite, maps the constant to the constant gt within
    1e-5 and keeps SSE(E) <= SSE(I).  An all-black render likewise: only b can move."""
    comp = torch.tensor([0.3, 0.5, 0.2]).repeat(20, 30, 1)
    gt = torch.tensor([0.45, 0.4, 0.35]).repeat(20, 30, 1)
    E = losses.colour_correction(comp, gt)
    assert bool(torch.isfinite(E).all())
    out = E[:, :3] @ comp[0, 0].double() + E[:, 3]
    assert float((out - gt[0, 0].double()).abs().max()) <= 1e-5
    assert ref.sse(comp, gt, E) <= ref.sse(comp, gt, ref.IDENTITY34)
    black = torch.zeros((20, 30, 3))
    E = losses.colour_correction(black, gt)
    assert bool(torch.isfinite(E).all()) and float((E[:, 3] - gt[0, 0].double()).abs().max()) <= 1e-5
    assert float((E[:, :3] - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12   # what the data do not show stays at the identity


def test_exact_affine_is_recovered_within_the_ridge_bound():
    rgba, gt = ref.images(37, 53, "iid", "black", noise=0.0)
    comp = ref.composite(rgba, "black")
    E = losses.colour_correction(comp, gt)
    mse = ref.sse(comp, gt, E) / (3 * 37 * 53)
    assert mse <= ref.ridge_bound(ref.E_TEST) + 1e-12, mse
    assert float(np.abs(E.numpy() - ref.E_TEST).max()) <= 1e-5
    assert ref.ridge_bound(ref.E_TEST) == pytest.approx(2.48e-8, rel=1e-3)


# ---- the trainer ----
class _RecordingEvaluator:
    """Records how it was called; returns the colour-corrected keys only when asked for them, as evaluate() does."""

    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, dict(kwargs)))
        n = len(args[2])
        res = dict(mean_psnr=20.0, mean_ssim=0.5, std_psnr=0.25, psnr=[20.0] * n, ssim=[0.5] * n, n_views=n)
        if kwargs.get("colour_corrected"):
            res.update(mean_cc_psnr=23.0, std_cc_psnr=0.125, mean_cc_ssim=0.625, cc_psnr=[23.0] * n, cc_ssim=[0.625] * n,
                       cc_mse=[0.005] * n, cc_l1=[0.05] * n, cc_transforms=[ref.IDENTITY34.tolist()] * n)
        return res


def _trainer(conf, stepper=None):
    conf = dict(conf, strategy=dict(method="GSStrategy"), out_dir="")
    ev = _RecordingEvaluator()
    tr = trainer_mod.Trainer(conf, None, _views(3), val_batches=_views(2), test_batches=_views(2), scene_extent=2.0,
                             stepper=stepper or _FakeStepper(_model()), strategy=_FakeStrategy(), evaluator=ev)
    return tr, ev


def test_option_off_calls_the_evaluator_as_before():
    conf = trainer_mod.resolve_config({})
    assert conf["evaluation"] == dict(colour_corrected=False, ridge=1e-6)
    assert trainer_mod.default_config("MCMCStrategy")["evaluation"] == dict(colour_corrected=False, ridge=1e-6)
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2))
    res = tr.run()
    assert len(ev.calls) == 2                                           # the validation at step 2 and the final test pass
    for args, kwargs in ev.calls:
        assert len(args) == 5 and kwargs == {}
    assert set(tr.validations[0]) == {"step", "loss", "mean_psnr", "mean_ssim", "n_gaussians"}
    assert "mean_cc_psnr" not in res["test"]


def test_option_on_adds_the_two_keywords_and_reports_the_means():
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2, evaluation=dict(colour_corrected=True, ridge=1e-5)))
    res = tr.run()
    assert len(ev.calls) == 2
    for args, kwargs in ev.calls:
        assert len(args) == 5 and kwargs == dict(colour_corrected=True, ridge=1e-5)
    assert ev.calls[0][0][3] is None and ev.calls[0][0][4] == 2 and ev.calls[1][0][4] == 4
    entry = tr.validations[0]
    assert entry["mean_cc_psnr"] == 23.0 and entry["mean_cc_ssim"] == 0.625 and entry["mean_psnr"] == 20.0
    assert res["test"]["mean_cc_psnr"] == 23.0 and res["test"]["std_cc_psnr"] == 0.125
    # composes with --exposure: the option needs nothing from the run's state or its checkpoint
    tr, ev = _trainer(dict(n_iterations=3, val_frequency=1000, exposure=dict(enabled=True), evaluation=dict(colour_corrected=True)),
                      stepper=_ExposureStepper(_model()))
    tr.run()
    assert ev.calls[-1][1] == dict(colour_corrected=True, ridge=1e-6)
    assert "evaluation" not in tr.checkpoint()["native"] and tr.checkpoint()["config"]["evaluation"]["colour_corrected"] is True


def test_command_line_switch_and_validation_of_the_block():
    ap = trainer_mod.build_parser()
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--cc-metrics"]))
    assert conf["evaluation"] == dict(colour_corrected=True, ridge=1e-6)
    assert conf["exposure"]["enabled"] is False                         # independent of --exposure
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--exposure"]))
    assert conf["evaluation"] == dict(colour_corrected=False, ridge=1e-6)
    trainer_mod.resolve_config(conf)
    for bad in (0.0, -1e-6, float("nan"), float("inf"), "1e-6", True):
        with pytest.raises(ValueError, match="ridge"):
            trainer_mod.resolve_config(dict(evaluation=dict(ridge=bad)))
    with pytest.raises(ValueError, match="colour_corrected"):
        trainer_mod.resolve_config(dict(evaluation=dict(colour_corrected="false")))
    with pytest.raises(ValueError, match="unknown"):
        trainer_mod.resolve_config(dict(evaluation=dict(color_corrected=True)))


def test_final_json_carries_the_corrected_means_only_when_present(monkeypatch, capsys):
    """main()'s last line: `test` gains mean_cc_psnr, std_cc_psnr and mean_cc_ssim when the evaluator returned them, and has exactly
    today's keys otherwise."""
    io_colmap = importlib.import_module("3dgrut_amd.io_colmap")

    class Scene:
        cameras_extent = 2.0

        def __init__(self, path, split, downsample, interval):
            self.n = 3 if split == "train" else 2

        def __len__(self):
            return self.n

        def batch(self, i):
            return _views(self.n)[i]

        def initial_gaussians(self, **kw):
            return None

    monkeypatch.setattr(io_colmap, "ColmapScene", Scene)
    real = trainer_mod.Trainer

    def fake_trainer(conf, init, tb, **kw):
        conf = dict(conf, n_iterations=2, out_dir="", strategy=dict(method="GSStrategy"))
        return real(conf, init, tb, stepper=_FakeStepper(_model()), strategy=_FakeStrategy(), evaluator=_RecordingEvaluator(), **kw)

    monkeypatch.setattr(trainer_mod, "Trainer", fake_trainer)
    assert trainer_mod.main(["--path", "x", "--cc-metrics"]) == 0
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last["test"] == dict(mean_psnr=20.0, std_psnr=0.25, mean_ssim=0.5, n_views=2, mean_cc_psnr=23.0, std_cc_psnr=0.125,
                                mean_cc_ssim=0.625)
    assert trainer_mod.main(["--path", "x"]) == 0
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last["test"] == dict(mean_psnr=20.0, std_psnr=0.25, mean_ssim=0.5, n_views=2)
