"""Pixel-weighted contribution scores and error-based densification without a GPU: the CPU reference of the weighted
walk against the plain one and against the oracle backward, the binding, select_by_error, the trainer's configuration and its
refusals, the mask forms of clone and split on the strategy golden inputs, the float64 definition of the error plane."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import weighted_contribution_reference as wr
from tests.common import check_gradient_rows
from tests.test_cpu_reference_pins import GOLD, _assert_stage, _StrategyStepper
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

capi = importlib.import_module("3dgrut_amd._capi")
losses = importlib.import_module("3dgrut_amd.losses")
strategy = importlib.import_module("3dgrut_amd.strategy")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_against_the_plain_walk_and_the_oracle_backward(name):
    """plane == 1: the weighted reference IS contribution_reference's weight_sum (the same float64 terms in the same order).  The
    seeded uniform plane: the sum equals the oracle backward's d(sum of P * red)/d(red feature) for the cotangent (P, 0, 0, 0), an
    independent statement of it, within that call's own flip budget and fp32 conditioning (common.check_gradient_rows)."""
    c, w = cr.case(name), wr.weighted_case(name)
    assert w["plane"].shape == (c["H"], c["W"]) and float(w["plane"].min()) >= 0.0 and float(w["plane"].max()) <= 1.0
    np.testing.assert_array_equal(w["ones_sum"], c["contrib"]["weight_sum"])
    assert (w["weighted_sum"] <= w["ones_sum"] + 1e-12).all() and (w["weighted_sum"] >= 0).all()
    assert ((w["weighted_sum"] > 0) == (w["ones_sum"] > 0)).all()        # (a uniform draw is never exactly 0)
    print(f"[weighted reference {name}] sum {w['weighted_sum'].sum():.6f} of {w['ones_sum'].sum():.6f}; vs the backward "
          f"{np.abs(w['weighted_sum'] - w['feat_grad']).max():.3e}")
    check_gradient_rows(w["weighted_sum"][:, None], w["feat_grad"][:, None], f"weighted reference {name}", budget=w["flip_budget"],
                        noise=w["fp32_noise"])


def test_reference_clamps_like_the_kernel():
    p = np.array([[-1.0, 0.0, 0.25], [1.0, 2.0, np.nan]])
    assert wr.clamp_plane(p).tolist() == [[0.0, 0.0, 0.25], [1.0, 1.0, 0.0]]


def test_binding():
    lib = capi.load()
    for sym in ("gut_trace_contribution_weighted", "gut_pixel_error"):
        assert sym in capi.EXPORTS and hasattr(lib, sym)
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gut_hip.h")).read()
    assert "int gut_trace_contribution_weighted(" in header and "int gut_pixel_error(" in header
    assert lib.gut_trace_contribution_weighted(None, None, 0, 3, 0, None, 8, 8, None, None, None, None, None, None) == 1
    assert b"gut_trace_contribution_weighted: null handle" in lib.gut_last_error()
    assert lib.gut_pixel_error(None, 8, 8, None, None, None, None, 0.0, None, None) == 1


def _result(err, pixels, weight=None):
    err = np.asarray(err, np.float64)
    return dict(weighted_sum=err, weight_sum=np.ones_like(err) if weight is None else np.asarray(weight, np.float64),
                max_weight=err.astype(np.float32), pixels=np.asarray(pixels, np.int64), n_views=1)


def test_select_by_error():
    sel = strategy.select_by_error
    r = _result([5, 1, 5, 0, 3, 5, 2, 0], [1, 1, 1, 9, 9, 1, 1, 0])
    # ceil(0.25 * 8) = 2; ties: the lower row first
    assert sel(r, 8, grow_fraction=0.25).tolist() == [True, False, True, False, False, False, False, False]
    assert sel(r, 8, grow_fraction=0.5).tolist() == [True, False, True, False, True, True, False, False]
    # zero scores are never selected, whatever the budget: 6 rows have a score
    assert sel(r, 8, grow_fraction=1.0).tolist() == [True, True, True, False, True, True, True, False]
    assert int(sel(r, 8, grow_fraction=0.0).sum()) == 0
    # min_pixels drops rows first
    assert sel(r, 8, grow_fraction=1.0, min_pixels=2).tolist() == [False, False, False, False, True, False, False, False]
    assert sel(_result([1, 2], [0, 0]), 2, grow_fraction=1.0, min_pixels=0).tolist() == [True, True]
    # the ceiling: ceil(0.3 * 8) = 3, ceil(0.1 * 30) = 3 although 0.1 * 30 > 3 in binary
    assert int(sel(r, 8, grow_fraction=0.3).sum()) == 3 == math.ceil(2.4)
    r30 = _result(np.arange(1, 31), np.ones(30))
    assert int(sel(r30, 30, grow_fraction=0.1).sum()) == 3 and sel(r30, 30, grow_fraction=0.1).tolist()[-3:] == [True] * 3
    # the room under max_n_gaussians
    assert int(sel(r, 8, grow_fraction=1.0, max_n_gaussians=10).sum()) == 2
    assert int(sel(r, 8, grow_fraction=1.0, max_n_gaussians=8).sum()) == 0 == int(sel(r, 8, grow_fraction=1.0, max_n_gaussians=5).sum())
    assert int(sel(r, 8, grow_fraction=0.25, max_n_gaussians=100).sum()) == 2
    # error_mean = weighted_sum / weight_sum, 0 where nothing was drawn
    rm = _result([4, 1, 3, 0, 2], [1, 1, 1, 1, 1], weight=[8, 1, 4, 0, 2])
    assert strategy.error_score_of(rm, "error_mean").tolist() == [0.5, 1.0, 0.75, 0.0, 1.0]
    assert sel(rm, 5, grow_fraction=0.4, score="error_mean").tolist() == [False, True, False, False, True]
    assert sel(rm, 5, grow_fraction=0.4, score="error_sum").tolist() == [True, False, True, False, False]
    # torch in, torch out; pure
    t = {k: (torch.as_tensor(v) if k != "n_views" else v) for k, v in r.items()}
    got = sel(t, 8, grow_fraction=0.5)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.bool and got.tolist() == sel(r, 8, grow_fraction=0.5).tolist()
    for bad in (dict(grow_fraction=1.5), dict(grow_fraction=-0.1), dict(score="weight_sum"), dict(min_pixels=-1), dict(min_pixels=0.5),
                dict(max_n_gaussians=-1)):
        with pytest.raises(ValueError):
            sel(r, 8, **bad)
    with pytest.raises(ValueError, match="must be"):
        sel(r, 7)
    with pytest.raises(ValueError, match="no weighted_sum"):
        sel({k: v for k, v in r.items() if k != "weighted_sum"}, 8)


def test_config_block_cli_and_refusals():
    conf = trainer_mod.resolve_config({})
    d = conf["strategy"]["densify"]
    assert d["criterion"] == "gradient"
    assert d["error"] == dict(grow_fraction=0.05, score="error_sum", min_pixels=1, views=0, max_n_gaussians=None)
    err = lambda **kw: dict(strategy=dict(densify=dict(criterion="error", **kw)))
    on = trainer_mod.resolve_config(err(error=dict(views=2, max_n_gaussians=1000)))
    assert on["strategy"]["densify"]["criterion"] == "error" and on["strategy"]["densify"]["error"]["views"] == 2
    for bad in (dict(grow_fraction=0.0), dict(grow_fraction=1.2), dict(grow_fraction="0.1"), dict(score="weight_sum"), dict(min_pixels=-1),
                dict(views=-1), dict(views=1.5), dict(max_n_gaussians=0), dict(unknown=1)):
        with pytest.raises(ValueError, match="strategy.densify.error"):
            trainer_mod.resolve_config(dict(strategy=dict(densify=dict(error=bad))))
    with pytest.raises(ValueError, match="strategy.densify.criterion must be one of"):
        trainer_mod.resolve_config(dict(strategy=dict(densify=dict(criterion="colour"))))
    # refused at configuration time: MCMC, the sorted variant, other kernel degrees, other split counts
    with pytest.raises(ValueError, match="GSStrategy only"):
        trainer_mod.resolve_config(dict(strategy=dict(method="MCMCStrategy", densify=dict(criterion="error"))))
    with pytest.raises(ValueError, match="unsorted variant"):
        trainer_mod.resolve_config(dict(err(), render=dict(splat=dict(k_buffer_size=16))))
    with pytest.raises(ValueError, match="particle_kernel_degree 2"):
        trainer_mod.resolve_config(dict(err(), render=dict(particle_kernel_degree=4)))
    with pytest.raises(ValueError, match="n_gaussians must be 2"):
        trainer_mod.resolve_config(err(split=dict(n_gaussians=3)))
    trainer_mod.resolve_config(dict(render=dict(particle_kernel_degree=4)))       # the gradient criterion takes them as before
    trainer_mod.resolve_config(dict(strategy=dict(method="MCMCStrategy")))
    ap = trainer_mod.build_parser()
    off = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert off["strategy"]["densify"] == conf["strategy"]["densify"]
    cli = trainer_mod.resolve_config(trainer_mod.config_from_args(ap.parse_args(
        ["--path", "x", "--densify-by", "error", "--densify-grow-fraction", "0.1", "--densify-views", "3"])))
    assert cli["strategy"]["densify"]["criterion"] == "error"
    assert cli["strategy"]["densify"]["error"] == dict(grow_fraction=0.1, score="error_sum", min_pixels=1, views=3, max_n_gaussians=None)
    assert cli["strategy"]["densify"]["frequency"] == 300
    with pytest.raises(ValueError, match="GSStrategy only"):
        trainer_mod.resolve_config(trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--strategy", "mcmc", "--densify-by", "error"])))


def test_trainer_refuses_the_criterion_on_several_gpus_and_installs_the_scorer():
    st = _FakeStepper(_model())
    st.world_size = 2
    conf = dict(n_iterations=1)
    with pytest.raises(ValueError, match="data-parallel error-based densification"):
        tr = trainer_mod.Trainer(dict(conf, strategy=dict(densify=dict(criterion="error"))), None, _trainer(conf)[0].train_batches,
                                 scene_extent=1.0, stepper=st, strategy=object())
    st = _FakeStepper(_model())
    st.resize_workspace = lambda: None
    gs = strategy.GSStrategy(st, criterion="error", grow_fraction=0.1, schedule=dict(strategy.GS_SCHEDULE, densify=(1, 100, 2)))
    tr = trainer_mod.Trainer(dict(conf, n_iterations=5, test_last=False, val_frequency=1000,
                                  strategy=dict(densify=dict(criterion="error", start_iteration=1, frequency=2, error=dict(views=2)))),
                             None, _trainer(conf)[0].train_batches, scene_extent=1.0, stepper=st, strategy=gs)
    assert gs.error_scorer == tr._score_error
    # views: all of them with 0, otherwise a function of (seed, step // frequency)
    assert tr._error_views(2) == trainer_mod.epoch_permutation(0, 1, 3)[:2] and tr._error_views(4) == trainer_mod.epoch_permutation(0, 2, 3)[:2]
    tr.conf["strategy"]["densify"]["error"]["views"] = 0
    assert tr._error_views(2) == [0, 1, 2]
    # the loop asks the scorer at the densify steps and the statistics say so
    asked = []

    def scorer(step):
        asked.append(step)
        n = st.model.num_gaussians
        return dict(weighted_sum=torch.arange(n, dtype=torch.float64), weight_sum=torch.ones(n, dtype=torch.float64),
                    pixels=torch.ones(n, dtype=torch.int64), n_views=1)
    gs.error_scorer = scorer
    gs.attach()
    assert getattr(st, "post_backward_hook", None) is None       # no statistics hook with this criterion
    stats = tr.train()
    assert asked == [2, 4]
    assert st.model.num_gaussians == 37 + 4 + 5 == 37 + math.ceil(3.7) + math.ceil(4.1)
    assert (stats["densify_criterion"], stats["densify_error_passes"], stats["densify_rows_added"]) == ("error", 2, 9)
    plain = _trainer(dict(n_iterations=2, val_frequency=1000))[0].train()
    assert not any(k.startswith("densify") for k in plain)


def _golden_strategy(**kw):
    S = np.load(os.path.join(GOLD, "strategy_golden.npz"))
    st = _StrategyStepper(S, "start")
    gs = strategy.GSStrategy(st, seed=0, **kw)
    unit, used = torch.as_tensor(S["unit_draws"]), []

    def draws(shape):
        used.append(shape[0])
        return unit[sum(used[:-1]):sum(used)]
    gs.unit_normal_fn = draws
    return S, st, gs, used


def test_mask_forms_of_clone_and_split_reproduce_the_gradient_criterion():
    """The strategy golden inputs (tests/test_cpu_reference_pins.py): the masks the gradient criterion forms from its statistics,
    handed to clone_rows / split_rows, leave the reference's rows, moments and draws."""
    S, st, gs, used = _golden_strategy()
    gs.attach()
    extent = float(S["scene_extent"])
    for g, s in zip(S["view_grads"], S["view_sensors"]):
        st.post_backward_hook(torch.as_tensor(g), torch.as_tensor(s))
    g = gs.grad_norm_accum / gs.grad_norm_denom
    g[g.isnan()] = 0.0
    g = g.squeeze(1)
    n0 = st.model.raw.shape[0]
    small = torch.exp(st.model.raw[:, 8:11]).max(dim=1).values <= gs.rel_size * extent
    clone_mask, split_mask = (g >= gs.clone_thr) & small, (g >= gs.split_thr) & ~small
    assert int(clone_mask.sum()) > 0 and int(split_mask.sum()) > 0
    assert gs.clone_rows(clone_mask) == int(clone_mask.sum())
    padded = torch.zeros(st.model.raw.shape[0], dtype=torch.bool)
    padded[:n0] = split_mask
    assert gs.split_rows(padded, step=600) == int(split_mask.sum())
    assert sum(used) == int(S["draws_used"])
    _assert_stage(S, "after_densify", st, gs, skip=("positions",))
    np.testing.assert_allclose(st.model.raw[:, 0:3].numpy(), S["after_densify/positions"], rtol=1e-5, atol=2e-7)


def test_densify_by_error_grows_one_row_per_selected_row():
    S, st, gs, used = _golden_strategy(criterion="error", grow_fraction=0.1)
    gs.attach()
    assert st.post_backward_hook is None and gs._rows_reordered in st.row_listeners
    extent = float(S["scene_extent"])
    raw0, feat0 = st.model.raw.clone(), st.model.features.clone()
    n = raw0.shape[0]
    score = torch.linspace(0.0, 1.0, n, dtype=torch.float64).flip(0)      # the first rows are the worst
    res = dict(weighted_sum=score, weight_sum=torch.ones(n, dtype=torch.float64), pixels=torch.ones(n, dtype=torch.int64), n_views=1)
    k = math.ceil(0.1 * n)
    small = (torch.exp(raw0[:, 8:11]).max(dim=1).values <= gs.rel_size * extent)[:k]
    assert gs.densify_by_error(res, extent, step=600) == k
    assert st.model.raw.shape[0] == n + k and st.m12.shape[0] == n + k and st.v48.shape[0] == n + k
    assert (gs.error_passes, gs.error_rows_added) == (1, k) and gs.grad_norm_accum.shape[0] == n + k
    n_small, n_big = int(small.sum()), int((~small).sum())
    assert sum(used) == 2 * n_big
    # the split parents left, everything else kept its order; then the clones; then the children (all parents, twice)
    kept = torch.ones(n, dtype=torch.bool)
    kept[:k] = small
    assert torch.equal(st.model.raw[:n - n_big], raw0[kept])
    assert torch.equal(st.model.raw[n - n_big:n - n_big + n_small], raw0[:k][small])
    assert torch.equal(st.model.features[n - n_big + n_small:], feat0[:k][~small].repeat(2, 1))
    assert float(st.m12[n - n_big:].abs().max()) == 0.0           # moments of new rows are zero
    with pytest.raises(RuntimeError, match="needs error_scorer"):
        gs.post_optimizer_step(600, extent)        # a densify step of the default schedule
    with pytest.raises(ValueError):
        strategy.GSStrategy(st, criterion="colour")
    with pytest.raises(ValueError):
        strategy.GSStrategy(st, criterion="error", split_n_gaussians=3)


def test_pixel_error_definition_on_hand_computed_pixels():
    """comp = rgb + B (1 - alpha); img = A comp + b; e = clamp(mean |img - gt|, 0, 1) * mask — four pixels by hand."""
    rgba = torch.tensor([[[0.2, 0.4, 0.6, 0.5], [0.1, 0.1, 0.1, 1.0]], [[0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 1.0]]])
    gt = torch.tensor([[[0.1, 0.1, 0.1], [0.1, 0.1, 0.1]], [[1.0, 1.0, 1.0], [0.5, 0.25, 0.0]]])
    e = losses.pixel_error(rgba, gt, "black")
    assert e.dtype == torch.float64 and tuple(e.shape) == (2, 2)
    f32 = lambda x: float(np.float32(x))
    want = [[(f32(0.2) - f32(0.1) + f32(0.4) - f32(0.1) + f32(0.6) - f32(0.1)) / 3, 0.0], [1.0, 0.25]]
    np.testing.assert_allclose(e.numpy(), want, rtol=0, atol=1e-15)
    # white background: pixel (0,0) gains 0.5 per channel, pixel (1,0) becomes white = its photo
    w = losses.pixel_error(rgba, gt, "white")
    np.testing.assert_allclose(w.numpy(), [[want[0][0] + 0.5, 0.0], [0.0, 0.25]], rtol=0, atol=1e-15)
    # a background plane, a mask, an exposure: E = [2 I | -0.1]
    B = torch.zeros(2, 2, 3)
    B[1, 0] = torch.tensor([1.0, 0.5, 0.0])
    np.testing.assert_allclose(losses.pixel_error(rgba, gt, B).numpy(), [[want[0][0], 0.0], [0.5, 0.25]], rtol=0, atol=1e-15)
    m = torch.tensor([[0.5, 1.0], [0.0, 1.0]])
    np.testing.assert_allclose(losses.pixel_error(rgba, gt, "black", mask=m).numpy(), [[want[0][0] / 2, 0.0], [0.0, 0.25]], rtol=0, atol=1e-15)
    E = torch.tensor([[2.0, 0, 0, -0.1], [0, 2.0, 0, -0.1], [0, 0, 2.0, -0.1]])
    x = losses.pixel_error(rgba, gt, "black", exposure=E)
    np.testing.assert_allclose(float(x[0, 1]), 0.0, atol=1e-7)                      # 2 * 0.1 - 0.1 = 0.1
    np.testing.assert_allclose(float(x[1, 1]), (0.4 + 0.65 + 0.9) / 3, atol=1e-7)
    # the clamp: an error above 1 counts as 1
    big = losses.pixel_error(torch.tensor([[[3.0, 3.0, 3.0, 1.0]]]), torch.zeros(1, 1, 3), 0.0)
    assert big.tolist() == [[1.0]]
