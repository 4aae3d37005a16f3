"""The attribute walk's backward and the feature fit without a GPU: the CPU reference of the gradient against the
oracle backward and as the adjoint of the attribute reference, the binding, the trainer's `features` block and the map loader, and
the reference fit's held-out condition."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import attribute_gradient_reference as gr
from tests import attribute_reference as ar
from tests import contribution_reference as cr
from tests.common import check_gradient_rows
from tests.test_cpu_masks import H, W, _colmap_dir
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

capi = importlib.import_module("3dgrut_amd._capi")
features = importlib.import_module("3dgrut_amd.features")
io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_against_the_oracle_backward(name):
    """The first three channels of the reference gradient are the oracle backward's d(sum of g . colour)/d(colour feature) for the
    cotangent (g_0, g_1, g_2, 0): an independent statement, within that call's own flip budget and fp32 conditioning
    (common.check_gradient_rows).  Rows nobody composited are exactly 0."""
    c, g = cr.case(name), gr.gradient_case(name)
    assert g["g"].shape == (4, c["H"], c["W"]) and float(g["g"].min()) < -0.9 and float(g["g"].max()) > 0.9
    assert g["grad"].shape == (c["d12"].shape[0], 4)
    print(f"[attribute gradient reference {name}] max |grad| {np.abs(g['grad']).max():.3f}; vs the backward "
          f"{np.abs(g['grad'][:, :3] - g['feat_grad']).max():.3e}; flip budget <= {g['flip_budget3'].max():.3e}, "
          f"noise <= {g['fp32_noise3'].max():.3e}")
    check_gradient_rows(g["grad"][:, :3], g["feat_grad"], f"attribute gradient reference {name}", budget=g["flip_budget3"],
                        noise=g["fp32_noise3"])
    assert not g["grad"][c["contrib"]["pixels"] == 0].any()
    assert float(g["grad"].min()) < 0 < float(g["grad"].max())


@pytest.mark.parametrize("name", cr.CASES)
def test_adjoint_identity(name):
    """sum_p g(p) . render(a)(p) = sum_i a_i . grad_i in float64, signed g and signed a, to 1e-9."""
    c, g = cr.case(name), gr.gradient_case(name)
    a = np.random.default_rng(130 + cr.case_index(name)).uniform(-1, 1, (c["d12"].shape[0], 4))
    planes = ar.attribute_reference(c["view"]["oracle_cam"], c["ref"], a, params=c["params"]())
    lhs, rhs = float((g["g"].astype(np.float64) * planes).sum()), float((a * g["grad"]).sum())
    print(f"[attribute gradient adjoint {name}] {lhs!r} vs {rhs!r}: difference {abs(lhs - rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-9 and abs(lhs) > 1e-3


def test_binding():
    lib = capi.load()
    assert "gut_trace_attributes_bwd" in capi.EXPORTS and hasattr(lib, "gut_trace_attributes_bwd")
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    assert len(lib.gut_trace_attributes_bwd.argtypes) == 14 == len(lib.gut_trace_attributes.argtypes)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gut_hip.h")).read()
    assert "int gut_trace_attributes_bwd(" in header
    assert lib.gut_trace_attributes_bwd(None, None, 0, 3, 0, None, 8, 8, None, None, None, 1, None, None) == 1
    assert b"gut_trace_attributes_bwd: null handle" in lib.gut_last_error()


def test_features_config_block_and_cli():
    conf = trainer_mod.resolve_config({})
    assert conf["features"] == dict(enabled=False, suffix="_features", iterations=200, lr=0.03)
    on = trainer_mod.resolve_config(dict(features=dict(enabled=True, iterations=5, lr=0.1)))
    assert on["features"] == dict(enabled=True, suffix="_features", iterations=5, lr=0.1)
    for bad in (dict(enabled=1), dict(suffix=""), dict(suffix=3), dict(iterations=0), dict(iterations=1.5), dict(iterations=True),
                dict(lr=0.0), dict(lr=-1.0), dict(lr="0.1"), dict(lr=float("nan")), dict(unknown=1)):
        with pytest.raises(ValueError, match="features"):
            trainer_mod.resolve_config(dict(features=bad))
    ap = trainer_mod.build_parser()
    off = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert off["features"] == conf["features"]
    cli = trainer_mod.resolve_config(trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--fit-features"])))
    assert cli["features"] == dict(enabled=True, suffix="_features", iterations=200, lr=0.03)
    cli = trainer_mod.resolve_config(trainer_mod.config_from_args(ap.parse_args(
        ["--path", "x", "--fit-features", "_dino", "--feature-iterations", "7", "--feature-lr", "0.5"])))
    assert cli["features"] == dict(enabled=True, suffix="_dino", iterations=7, lr=0.5)


def test_trainer_refuses_features_on_several_gpus_and_without_maps():
    st = _FakeStepper(_model())
    st.world_size = 2
    conf = dict(n_iterations=1)
    with pytest.raises(ValueError, match="data-parallel feature fitting"):
        trainer_mod.Trainer(dict(conf, features=dict(enabled=True)), None, _trainer(conf)[0].train_batches, scene_extent=1.0, stepper=st,
                            strategy=object())
    tr = _trainer(dict(conf, features=dict(enabled=True)))[0]
    with pytest.raises(ValueError, match="no training view has a target map"):
        tr.fit_features()


def test_feature_map_loader(tmp_path):
    """`<image stem><suffix>.npy`: float [K,H,W] or [H,W] (one channel) at the image's size, returned as float32 [K,H,W]; None
    without the file; every other shape, type or size is refused."""
    root = _colmap_dir(str(tmp_path))
    scene = io_colmap.ColmapScene(root, "train", 1, test_split_interval=0)
    stem = os.path.join(root, "images", "a")
    assert scene.load_feature_map(0, "_features") is None
    np.save(stem + "_features.npy", np.arange(3 * H * W, dtype=np.float64).reshape(3, H, W))
    m = scene.load_feature_map(0, "_features")
    assert m.dtype == np.float32 and m.shape == (3, H, W) and m[2, H - 1, W - 1] == 3 * H * W - 1 and m.flags["C_CONTIGUOUS"]
    np.save(stem + "_one.npy", np.ones((H, W), np.float32))
    assert scene.load_feature_map(0, "_one").shape == (1, H, W)
    assert scene.load_feature_map(1, "_features") is None
    for bad in (np.ones((3, H, W - 1), np.float32), np.ones((3, H // 2, W), np.float32), np.ones((W,), np.float32),
                np.ones((2, 3, H, W), np.float32), np.ones((3, H, W), np.int32), np.ones((65, H, W), np.float32),
                np.full((1, H, W), np.nan, np.float32), np.ones((3, W, H), np.float32)):
        np.save(stem + "_bad.npy", bad)
        with pytest.raises(ValueError, match="feature map"):
            scene.load_feature_map(0, "_bad")
    with pytest.raises(ValueError, match="feature map"):
        scene.load_feature_map(0, "_features", size=(W // 2, H // 2))
    # the downsampled folder has its own maps at its own size
    half = io_colmap.ColmapScene(root, "train", 2, test_split_interval=0)
    np.save(os.path.join(root, "images_2", "a_features.npy"), np.zeros((2, H // 2, W // 2), np.float32))
    assert half.load_feature_map(0, "_features").shape == (2, H // 2, W // 2)


def test_feature_targets_are_checked():
    class R:
        act = torch.zeros((5, 12))
    with pytest.raises(ValueError, match="views and"):
        features.fit_features(R(), [1, 2], [torch.zeros(2, 4, 4)], 2, 1, 0.1)
    with pytest.raises(ValueError, match="target map must be"):
        features.fit_features(R(), [1], [torch.zeros(3, 4, 4)], 2, 1, 0.1)
    with pytest.raises(ValueError, match="between 1 and 64"):
        features.fit_features(R(), [1], [torch.zeros(3, 4, 4)], 0, 1, 0.1)
    with pytest.raises(ValueError, match="init must be"):
        features.fit_features(R(), [1], [torch.zeros(2, 4, 4)], 2, 1, 0.1, init=torch.zeros(4, 2))
    out, alpha, target = torch.ones(2, 3, 3), torch.full((3, 3), 0.5), torch.full((2, 3, 3), 4.0)
    assert float(features.default_loss(out, alpha, target)) == 1.0


def test_reference_fit_generalises_to_the_held_out_view():
    """Adam at 0.03 from zero, 200 iterations alternating the two fitted views, float64: the held-out view's MSE is at most 1e-2 of
    the zero fit's, and every row is seen by the two fitted views."""
    f = gr.fit_case()
    print(f"[reference feature fit] held-out MSE {f['heldout_mse']:.3e} against the zero fit's {f['zero_mse']:.3e}: "
          f"{f['heldout_mse'] / f['zero_mse']:.3e} x; {int(f['seen'].sum())} of {f['seen'].size} rows seen")
    assert f["heldout_mse"] <= 1e-2 * f["zero_mse"]
    assert bool(f["seen"].all())
    for r, al, m in zip(f["rendered"], f["alphas"], f["maps"]):
        np.testing.assert_allclose(al[None] * m, r, rtol=0, atol=1e-12)
