"""Error-based densification in the trainer (strategy.densify.criterion: error) on the synthetic COLMAP scene, with
the initial points thinned to a seeded 1 in 8 wherever x > 0: the half of the scene that lacks Gaussians is where the rendering
error is, and where the rows should be added.  120 iterations, densify start 50 and frequency 50 (one densify step, at 100)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

strategy_mod = importlib.import_module("3dgrut_amd.strategy")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")

PLAIN_KEYS = {"n_steps", "n_epochs", "steps_run", "training_time", "iteration_speed", "n_gaussians"}


@pytest.fixture(scope="module")
def thinned_scene(tmp_path_factory):
    from tests.synthetic_colmap import load_scene, write_synthetic_colmap
    root = write_synthetic_colmap(str(tmp_path_factory.mktemp("synthetic_colmap_error_densify")))
    init, tb, vb, extent = load_scene(root)
    n = init["positions"].shape[0]
    x = np.asarray(init["positions"])[:, 0]
    keep = (x <= 0) | (np.random.default_rng(8).random(n) < 1.0 / 8.0)
    thinned = {k: (v[keep] if hasattr(v, "shape") and v.shape[:1] == (n,) else v) for k, v in init.items()}
    assert 0 < int((x[keep] > 0).sum()) < int((x[keep] <= 0).sum()) // 4
    return root, thinned, tb, vb, extent


def _conf(root, args, out_dir=""):
    conf = trainer_mod.config_from_args(trainer_mod.build_parser().parse_args(["--path", root, "--n-iterations", "120"] + args))
    conf["strategy"]["densify"].update(start_iteration=50, frequency=50)
    conf["out_dir"] = out_dir
    return conf


def _run(scene, args, out_dir="", at_random=False, monkeypatch=None):
    """One run; returns (result, [(N before, x > 0 before, selected, N after, x > 0 after)] per error-densify step)."""
    root, init, tb, vb, extent = scene
    tr = trainer_mod.Trainer(_conf(root, args, out_dir), init, tb, val_batches=vb, test_batches=vb, scene_extent=extent)
    passes = []
    by_error = getattr(tr.strategy, "densify_by_error")

    def recorded(result, scene_extent, step=0):
        raw = tr.model.raw
        before = (int(raw.shape[0]), int((raw[:, 0] > 0).sum()))
        k = by_error(result, scene_extent, step)
        raw = tr.model.raw
        passes.append((*before, k, int(raw.shape[0]), int((raw[:, 0] > 0).sum())))
        return k
    tr.strategy.densify_by_error = recorded
    if at_random:
        by_score = strategy_mod.select_by_error

        def uniformly(result, n, *a, **kw):
            k = int(by_score(result, n, *a, **kw).sum())
            mask = torch.zeros(n, dtype=torch.bool)
            mask[torch.randperm(n, generator=torch.Generator().manual_seed(7))[:k]] = True
            return mask.to(result["pixels"].device)
        monkeypatch.setattr(strategy_mod, "select_by_error", uniformly)
    try:
        return tr.run(), passes
    finally:
        if at_random:
            monkeypatch.undo()


def test_trainer_densifies_where_the_error_is_and_its_checkpoint_resumes(thinned_scene, tmp_path, monkeypatch):
    root, init, tb, vb, extent = thinned_scene
    args = ["--densify-by", "error", "--densify-grow-fraction", "0.1"]
    scored, passes = _run(thinned_scene, args, out_dir=str(tmp_path))
    s = scored["stats"]
    print(f"[error densify] passes (N, x>0, selected, N after, x>0 after): {passes}\n[error densify] {json.dumps(s)}")
    assert len(passes) == 1                                      # the densify step at 100
    for n0, _, k, n1, _ in passes:
        assert k == int(np.ceil(0.1 * n0 - 1e-9)) and n1 == n0 + k   # a clone and a two-way split are each +1
    assert s["densify_criterion"] == "error" and s["densify_error_passes"] == len(passes)
    assert s["densify_rows_added"] == sum(p[3] - p[0] for p in passes) and s["n_gaussians"] == passes[-1][3]
    assert set(s) == PLAIN_KEYS | {"densify_criterion", "densify_error_passes", "densify_rows_added"}
    # where the rows went: the share of the net added rows with x > 0 against the share of x > 0 rows just before the first pass,
    # which is what a uniformly random choice of rows would give
    n0, pos0 = passes[0][0], passes[0][1]
    added = sum(p[3] - p[0] for p in passes)
    added_pos = sum(p[4] - p[1] for p in passes)
    print(f"[error densify] x > 0: {pos0} of {n0} rows before ({pos0 / n0:.3f}), {added_pos} of the {added} added rows ({added_pos / added:.3f})")
    assert added_pos / added > pos0 / n0
    # the checkpoint holds nothing of the scores and resumes
    path = os.path.join(str(tmp_path), "ckpt_last.pt")
    ckpt = torch.load(path, weights_only=True)
    n = s["n_gaussians"]
    assert ckpt["positions"].shape[0] == n and ckpt["global_step"] == 120
    assert not any("error" in k or "weighted" in k for k in ckpt) and not any("error" in k or "weighted" in k for k in ckpt["native"])
    conf = _conf(root, args)
    conf.update(n_iterations=125, resume=path, test_last=False, val_frequency=10 ** 9)
    resumed = trainer_mod.Trainer(conf, None, tb, test_batches=vb, scene_extent=extent)
    assert resumed.model.num_gaussians == n and resumed.global_step == 120 and resumed.strategy.criterion == "error"
    resumed.train()
    assert resumed.global_step == 125 and bool(torch.isfinite(resumed.model.raw).all())

    # a run without the flag has exactly today's statistic keys
    plain, none = _run(thinned_scene, [])
    assert set(plain["stats"]) == PLAIN_KEYS and none == []

    # a measurement, not an assertion: the same number of rows chosen uniformly at random (seeded)
    chance, chance_passes = _run(thinned_scene, args, at_random=True, monkeypatch=monkeypatch)
    assert [p[2] for p in chance_passes] == [p[2] for p in passes]
    print(f"[error densify] held-out PSNR after 120 iterations: rows by error {scored['test']['mean_psnr']:.3f}, the same number at random "
          f"{chance['test']['mean_psnr']:.3f}, gradient criterion {plain['test']['mean_psnr']:.3f} (N {s['n_gaussians']}, "
          f"{chance['stats']['n_gaussians']}, {plain['stats']['n_gaussians']})")
