"""Contribution scores without a GPU: the CPU reference's identities and the preconditions of the GPU cases
(tests/contribution_reference.py), keep_mask's host logic, compact() and the trainer's compaction step on the fake stepper, the
binding."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

capi = importlib.import_module("3dgrut_amd._capi")
contribution = importlib.import_module("3dgrut_amd.contribution")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_identities(name):
    """sum_i weight_sum_i = sum of the alpha plane, sum_i pixels_i = sum of the hit-count plane exactly, and the per-Gaussian sum is
    the oracle backward's d(sum of red)/d(red feature): a second, independent statement of it.  Measured on the 64 x 48 pinhole case:
    999.01806 against 999.01807, 13894 and 13894, 1.3e-7 absolute.  The bounds: the planes are float32 (2^-23 relative per pixel sum,
    rounded up to 1e-6 of the total), the two float64 sums of float32-evaluated terms agree to 1e-6 of the largest row."""
    c = cr.case(name)
    k, ref = c["contrib"], c["ref"]
    alpha = float(ref["rgba"][..., 3].astype(np.float64).sum())
    print(f"[reference {name}] sum weight_sum {k['weight_sum'].sum():.6f} vs sum alpha {alpha:.6f}; pixels {int(k['pixels'].sum())} vs hits "
          f"{float(ref['hits'].sum()):.0f}; per-Gaussian vs backward {np.abs(k['weight_sum'] - c['feat_grad']).max():.3e}")
    assert abs(k["weight_sum"].sum() - alpha) <= 1e-6 * alpha
    assert int(k["pixels"].sum()) == int(ref["hits"].astype(np.float64).sum())
    assert np.abs(k["weight_sum"] - c["feat_grad"]).max() <= 1e-6 * np.abs(c["feat_grad"]).max()
    assert (k["max_weight"] <= 1.0).all() and (k["max_weight_calm"] <= k["max_weight"]).all()
    assert ((k["pixels"] > 0) == (k["max_weight"] > 0)).all()


@pytest.mark.parametrize("name", cr.CASES)
def test_gpu_cases_say_something(name):
    """Every GPU case scores at least 100 Gaussians, and at least half of the scored ones have neither a flip budget nor a prone
    entry: on them the GPU test is an exact statement (pixels) or an fp32 one (sums, maxima).  Every case but the 64 x 48 pinhole
    one — whose 300 Gaussians are all composited somewhere: measured, and asserted so that it is noticed if it changes — also has
    a Gaussian with a tile and no composited pixel, the rows the "unwalked or unscored rows stay zero" checks are about."""
    c = cr.case(name)
    k, ref = c["contrib"], c["ref"]
    scored = k["pixels"] > 0
    clean = scored & (c["flip_budget"] == 0) & (k["prone_entries"] == 0)
    listed_unscored = int(((ref["tiles_count"] > 0) & ~scored).sum())
    print(f"[cases {name}] {int(scored.sum())} scored, {int(clean.sum())} clean, {k['prone_pixels']} prone pixels, "
          f"{int((c['flip_budget'] > 0).sum())} with a flip budget, {listed_unscored} with a tile and no pixel")
    assert int(scored.sum()) >= 100
    assert 2 * int(clean.sum()) >= int(scored.sum())
    if name == "pinhole_64x48":
        assert listed_unscored == 0 and int(scored.sum()) == 300
    else:
        assert listed_unscored >= 1
    if name == "single_tile_1025":
        lens = (ref["tile_ranges"][:, 1] - ref["tile_ranges"][:, 0]).tolist()
        assert lens == [1025]      # one tile, more than 512 entries: chunk and selection boundaries inside the walk


def _result(scores, pixels):
    return dict(weight_sum=np.asarray(scores, np.float64), max_weight=np.asarray(scores, np.float32), pixels=np.asarray(pixels, np.int64), n_views=1)


def test_keep_mask_counts_ties_and_min_pixels():
    r = _result([5, 1, 5, 0, 3, 5, 2], [1, 1, 1, 0, 9, 1, 1])
    km = contribution.keep_mask
    assert km(r, keep_count=2).tolist() == [True, False, True, False, False, False, False]        # ties: the lower row first
    assert km(r, keep_count=4).tolist() == [True, False, True, False, True, True, False]
    assert km(r, keep_count=7).all() and not km(r, keep_count=0).any()
    assert km(r, min_pixels=1).tolist() == [True, True, True, False, True, True, True]             # neither selector: min_pixels only
    assert km(r).all()
    assert km(r, keep_count=7, min_pixels=1).tolist() == [True, True, True, False, True, True, True]   # fewer eligible rows than the count
    assert km(r, keep_count=1, min_pixels=2).tolist() == [False, False, False, False, True, False, False]   # dropped first, then the best
    assert km(r, keep_fraction=0.5).sum() == 4 == math.ceil(3.5)                                   # ceil
    assert km(r, keep_fraction=1.0 / 7.0).sum() == 1 and km(r, keep_fraction=1.0).all()
    assert contribution.keep_count_of(0.1, 30) == 3 and contribution.keep_count_of(0.5, 9223) == 4612
    assert km(r, score="max_weight", keep_count=3).tolist() == km(r, keep_count=3).tolist()
    t = {k: (torch.as_tensor(v) if k != "n_views" else v) for k, v in r.items()}
    got = km(t, keep_count=4)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.bool and got.tolist() == km(r, keep_count=4).tolist()
    for _ in range(2):
        assert km(r, keep_fraction=0.4).tolist() == km(r, keep_fraction=0.4).tolist()


def test_keep_mask_refusals():
    r = _result([1, 2, 3], [1, 1, 1])
    with pytest.raises(ValueError, match="not both"):
        contribution.keep_mask(r, keep_fraction=0.5, keep_count=1)
    for bad in (dict(score="pixels"), dict(keep_fraction=1.5), dict(keep_fraction=-0.1), dict(keep_count=4), dict(keep_count=-1),
                dict(keep_count=1.5), dict(min_pixels=-1), dict(min_pixels=0.5)):
        with pytest.raises(ValueError):
            contribution.keep_mask(r, **bad)


def test_binding_and_record_layout():
    lib = capi.load()
    assert "gut_trace_contribution" in capi.EXPORTS and hasattr(lib, "gut_trace_contribution")
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    assert C.sizeof(capi.GutContribution) == 16
    assert [(f, getattr(capi.GutContribution, f).offset) for f, _ in capi.GutContribution._fields_] == \
        [("weight_sum_q32", 0), ("max_weight_bits", 8), ("pixels", 12)]
    assert lib.gut_trace_contribution(None, None, 0, 3, 0, None, 8, 8, None, None, None, None) == 1
    assert b"gut_trace_contribution: null handle" in lib.gut_last_error()


def test_unpack_scores():
    rec = np.zeros(3, dtype=[("q", "<u8"), ("m", "<u4"), ("p", "<u4")])
    rec["q"] = [0, 3 << 31, (255 << 32) + 1]
    rec["m"] = np.array([0.0, 0.75, 0.99], np.float32).view(np.uint32)
    rec["p"] = [0, 7, 0xFFFFFFF0]
    ws, mw, px = contribution.unpack_scores(torch.as_tensor(rec.view(np.int64).reshape(3, 2)))
    assert ws.dtype == torch.float64 and ws.tolist() == [0.0, 1.5, 255.0 + 2.0 ** -32]
    assert mw.dtype == torch.float32 and mw.tolist() == [0.0, 0.75, float(np.float32(0.99))]
    assert px.dtype == torch.int64 and px.tolist() == [0, 7, 0xFFFFFFF0]


def test_compact_moves_parameters_and_moments_together():
    model = _model(37)
    st = _FakeStepper(model)
    st.resize_workspace = lambda: None
    synced = []
    st.sync_moments = lambda: synced.append(model.raw.shape[0])
    raw, feat, m12, v48 = model.raw.clone(), model.features.clone(), st.m12.clone(), st.v48.clone()
    mask = torch.arange(37) % 3 != 1
    removed = contribution.compact(st, mask)
    assert removed == 12 and model.raw.shape[0] == 25 and synced and synced[0] == 37    # moments brought up to date BEFORE rows move
    assert torch.equal(model.raw, raw[mask]) and torch.equal(model.features, feat[mask])
    assert torch.equal(st.m12, m12[mask]) and torch.equal(st.v48, v48[mask]) and st.v12.shape[0] == 25 and st.m48.shape[0] == 25
    assert model.raw[:, 11].tolist() == [float(i) for i in range(37) if i % 3 != 1]       # order kept
    with pytest.raises(ValueError, match="mask must be"):
        contribution.compact(st, torch.ones(37, dtype=torch.bool))


def test_config_block_and_cli():
    conf = trainer_mod.resolve_config({})
    assert conf["compaction"] == dict(enabled=False, keep_fraction=0.5, score="weight_sum", min_pixels=1, finetune_iterations=0)
    for bad in (dict(enabled="false"), dict(keep_fraction=0.0), dict(keep_fraction=1.2), dict(score="pixels"), dict(min_pixels=-1),
                dict(finetune_iterations=1.5), dict(unknown=1)):
        with pytest.raises(ValueError, match="compaction"):
            trainer_mod.resolve_config(dict(compaction=bad))
    ap = trainer_mod.build_parser()
    off = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert off["compaction"] == conf["compaction"]
    on = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--compact-to", "0.25", "--compact-score", "max_weight", "--compact-finetune", "20"]))
    assert on["compaction"] == dict(enabled=True, keep_fraction=0.25, score="max_weight", min_pixels=1, finetune_iterations=20)


def test_trainer_without_the_block_calls_what_it_called():
    tr, st, strat, ev, saved = _trainer(dict(n_iterations=5, val_frequency=1000, test_last=True))
    tr.test_batches = list(tr.val_batches)
    tr.compact = lambda: pytest.fail("compaction ran although the block is off")
    res = tr.run()
    assert len(st.steps) == 5 and ev.steps == [5] and saved == [5]
    assert not any(k.startswith("compaction") for k in res["stats"])
    assert set(res["stats"]) == {"n_steps", "n_epochs", "steps_run", "training_time", "iteration_speed", "n_gaussians"}


def test_trainer_compaction_step_order(monkeypatch):
    """Block on, with the scorer replaced: test pass before, scores over the training views in order, pruning through compact(),
    the fine-tuning steps without the strategy, then the usual checkpoint and test pass; the four new statistics."""
    tr, st, strat, ev, saved = _trainer(dict(n_iterations=4, val_frequency=1000, test_last=True,
                                             compaction=dict(enabled=True, keep_fraction=0.5, finetune_iterations=3)))
    tr.test_batches = list(tr.val_batches)
    st.resize_workspace = lambda: None
    seen = []

    class Scorer:
        def __init__(self, model, tracer):
            self.n = model.num_gaussians

        def accumulate(self, batch):
            seen.append(batch.tag)

        def result(self):
            w = torch.arange(self.n, dtype=torch.float64)
            return dict(weight_sum=w, max_weight=w.float(), pixels=torch.ones(self.n, dtype=torch.int64), n_views=len(seen))
    monkeypatch.setattr(contribution, "ContributionScores", Scorer)
    res = tr.run()
    assert seen == [0, 1, 2]
    assert ev.steps == [4, 7] and saved == [7] and tr.global_step == 7
    assert [s for s, _ in st.steps] == list(range(7)) and len(strat.calls) == 4          # no strategy call while fine-tuning
    assert tr.model.num_gaussians == 19 == math.ceil(0.5 * 37) and st.m12.shape[0] == 19 and st.v48.shape[0] == 19
    assert tr.model.raw[:, 11].tolist() == [float(i) for i in range(18, 37)]             # the 19 best rows, in their order
    s = res["stats"]
    assert (s["compaction_n_before"], s["compaction_n_after"], s["compaction_score"], s["compaction_test_psnr_before"]) == (37, 19, "weight_sum", 20.0)
    assert s["n_gaussians"] == 19


def test_trainer_refuses_the_block_on_several_gpus():
    st = _FakeStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError, match="compaction: data-parallel"):
        _trainer(dict(n_iterations=1, compaction=dict(enabled=True)), stepper=st)
