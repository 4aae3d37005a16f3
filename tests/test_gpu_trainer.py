"""The end-to-end Trainer on a synthetic COLMAP scene (tests/synthetic_colmap.py: a 200 k-Gaussian teacher rendered from 32 orbit views
at 400x400; every 8th view held out): lazy moments, the fused loss, densify / prune / density reset, the SH ramp and the position-lr
decay running together, and the held-out PSNR they reach.  The bars were set from one MI355X run each, at the measured value minus a
stated margin (values in the docstrings).  Repeat-to-repeat spread of the native run (float atomics in the compositing backward):
0.008 dB between two 1 200-step runs that differ only by a checkpoint / resume at step 600, 0.001 dB between the native trainer and
the autograd path; both below 0.1 dB, so the tolerance of the issue, 0.3 dB, stands."""
import collections
import importlib
import os
import subprocess
import sys

import pytest
import torch

from tests.synthetic_colmap import load_scene, write_synthetic_colmap

pytestmark = pytest.mark.gpu
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
evaluate = importlib.import_module("3dgrut_amd.evaluate").evaluate
schedule = importlib.import_module("3dgrut_amd.schedule")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def colmap_dir(tmp_path_factory):
    return write_synthetic_colmap(str(tmp_path_factory.mktemp("synthetic_colmap")))


def _counting(obj, names):
    counts = collections.Counter()
    for name in names:
        fn = getattr(obj, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            counts[_name] += 1
            return _fn(*a, **k)
        setattr(obj, name, wrapped)
    return counts


def _fired(stage, n):
    return sum(schedule.check_step_condition(g, *stage) for g in range(n))


NO_EVENTS = dict(densify=dict(start_iteration=-1, end_iteration=-1), prune=dict(start_iteration=-1, end_iteration=-1),
                 reset_density=dict(start_iteration=-1, end_iteration=-1))


def _gs_conf(n, out_dir="", **kw):
    """gs.yaml compressed onto n steps: densify and prune from 300 to 2/3 n, density reset every 0.3 n, the SH degree every 0.2 n
    (reaching 3), the position rate at lr_final after the last step."""
    end = 2 * n // 3
    conf = dict(n_iterations=n, val_frequency=n // 6, validate_first=True, test_last=True, out_dir=out_dir,
                checkpoint=dict(iterations=[]), model=dict(progressive_training=dict(increase_frequency=n // 5)),
                scheduler=dict(positions=dict(max_steps=n - 1)),
                strategy=dict(method="GSStrategy", densify=dict(start_iteration=300, end_iteration=end, frequency=300),
                              prune=dict(start_iteration=300, end_iteration=end, frequency=100),
                              reset_density=dict(start_iteration=0, end_iteration=end, frequency=3 * n // 10)))
    return trainer_mod._merge(conf, kw)


def test_acceptance_gs_run(colmap_dir, tmp_path):
    """3 000 steps of the GS recipe.  Measured on MI355X: held-out PSNR 12.91 dB at step 0 (validate_first), 22.44 dB after the run
    (SSIM 0.596); N 20 000 -> 46 101 (densify at 600 .. 1800, prune every 100 steps, density reset at 900 and 1800); 1 301 it/s
    including every validation and densification event."""
    init, tb, vb, extent = load_scene(colmap_dir)
    conf = _gs_conf(3000, out_dir=str(tmp_path))
    tr = trainer_mod.Trainer(conf, init, tb, val_batches=vb, test_batches=vb, scene_extent=extent)
    n0 = tr.model.num_gaussians
    counts = _counting(tr.strategy, ("densify", "prune_opacity", "reset_density"))
    res = tr.run()
    sched = trainer_mod.gs_schedule(tr.conf)
    for name, stage in (("densify", "densify"), ("prune_opacity", "prune"), ("reset_density", "reset_density")):
        assert counts[name] == _fired(sched[stage], 3000) >= 2, (name, counts)
    traj = [v["n_gaussians"] for v in tr.validations] + [tr.model.num_gaussians]
    first, final = tr.validations[0]["mean_psnr"], res["test"]["mean_psnr"]
    print(f"\n[acceptance] iteration_speed {res['stats']['iteration_speed']:.1f} it/s, training_time {res['stats']['training_time']:.2f} s, "
          f"N {n0} -> {traj}, psnr first {first:.3f} final {final:.3f} ssim {res['test']['mean_ssim']:.4f}, "
          f"val {[round(v['mean_psnr'], 2) for v in tr.validations]}")
    assert tr.model.num_gaussians != n0
    assert torch.isfinite(tr.model.raw).all() and torch.isfinite(tr.model.features).all()
    assert all(v["loss"] is None or v["loss"] == v["loss"] for v in tr.validations)
    assert tr.model.n_active_features == 3
    assert float(tr.stepper.lr12[0]) == pytest.approx(0.0000016 * extent, rel=1e-5)
    assert res["stats"]["iteration_speed"] > 0 and res["stats"]["n_steps"] == 3000
    assert os.path.isfile(os.path.join(str(tmp_path), "ckpt_last.pt"))
    assert os.path.isfile(os.path.join(str(tmp_path), "ours_3000", "renders", "00000.png"))
    assert first < final - FIRST_PSNR_MARGIN
    assert final >= FINAL_PSNR_BAR


FINAL_PSNR_BAR = 22.44 - 1.0      # measured final held-out PSNR minus a 1 dB margin
FIRST_PSNR_MARGIN = 9.5 - 3.5     # measured gain over the untrained model (9.5 dB) minus a 3.5 dB margin


def test_mcmc_run(colmap_dir):
    """600 steps of the MCMC recipe with relocate / add every 100 steps up to a cap of 1.15 N0.  Measured on MI355X: N 20 000 -> 23 000
    (the cap), held-out PSNR 20.00 dB."""
    train = importlib.import_module("3dgrut_amd.io_colmap").ColmapScene(colmap_dir, "train", 1, 8)
    conf = trainer_mod.default_config("MCMCStrategy")
    init = train.initial_gaussians(default_density=conf["model"]["default_density"], default_scale_factor=conf["model"]["default_scale_factor"])
    _, tb, vb, extent = load_scene(colmap_dir)
    n0 = init["positions"].shape[0]
    cap = int(1.15 * n0)
    conf = trainer_mod._merge(conf, dict(n_iterations=600, val_frequency=10 ** 9, test_last=True, out_dir="",
                                         scheduler=dict(positions=dict(max_steps=599)), model=dict(progressive_training=dict(increase_frequency=200)),
                                         strategy=dict(relocate=dict(start_iteration=100, end_iteration=500, frequency=100),
                                                       add=dict(start_iteration=100, end_iteration=500, frequency=100, max_n_gaussians=cap))))
    tr = trainer_mod.Trainer(conf, init, tb, val_batches=vb, test_batches=vb, scene_extent=extent)
    counts = _counting(tr.strategy, ("relocate", "add_new"))
    sizes = []
    post = tr.strategy.post_optimizer_step

    def watch(step, lr):
        out = post(step, lr)
        sizes.append(tr.model.num_gaussians)
        return out
    tr.strategy.post_optimizer_step = watch
    res = tr.run()
    final = res["test"]["mean_psnr"]
    print(f"\n[mcmc] N {n0} -> {tr.model.num_gaussians} (cap {cap}), psnr {final:.3f}, {res['stats']['iteration_speed']:.1f} it/s")
    sched = trainer_mod.mcmc_schedule(tr.conf)
    assert counts["relocate"] == _fired(sched["relocate"], 600) >= 2 and counts["add_new"] == _fired(sched["add"], 600) >= 2
    assert max(sizes) <= cap and tr.model.num_gaussians > n0
    assert torch.isfinite(tr.model.raw).all()
    assert final >= MCMC_PSNR_BAR


MCMC_PSNR_BAR = 20.00 - 1.0       # measured held-out PSNR minus a 1 dB margin


def test_native_trainer_matches_the_reference_surface(colmap_dir, gut):
    """Same init, views and view order, no densification, 1 000 steps: Trainer against a loop over train.TrainStep
    (Tracer.render -> autograd -> torch.optim.Adam).  Measured on MI355X: 21.227 dB native, 21.226 dB reference surface."""
    train = importlib.import_module("3dgrut_amd.train")
    model_mod = importlib.import_module("3dgrut_amd.model")
    init, tb, vb, extent = load_scene(colmap_dir)
    conf = dict(n_iterations=1000, val_frequency=10 ** 9, test_last=False, out_dir="", strategy=dict(method="GSStrategy", **NO_EVENTS))
    tr = trainer_mod.Trainer(conf, init, tb, test_batches=vb, scene_extent=extent)
    tr.train()
    ours = evaluate(tr.model, tr.tracer, vb)["mean_psnr"]
    c = tr.conf
    model = model_mod.GaussianModel(init, sh_degree=0)
    sched = schedule.TrainSchedule(extent, lr_final=c["scheduler"]["positions"]["lr_final"], max_steps=c["scheduler"]["positions"]["max_steps"])
    tracer = gut.Tracer({"render": {}})
    ts = train.TrainStep(model, tracer, scene_extent=extent, schedule=sched)
    for g in range(1000):
        ts.step(tb[tr.batch_index(g)])
    ref = evaluate(model, tracer, vb)["mean_psnr"]
    print(f"\n[native vs reference surface] psnr native {ours:.4f} reference {ref:.4f}")
    assert abs(ours - ref) <= PSNR_TOL


PSNR_TOL = 0.3   # the issue's tolerance; the measured spread (module docstring) is below 0.1 dB


def _equal(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _equal(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


def test_resume_continues_the_run(colmap_dir, tmp_path):
    """1 200 steps straight against 600 steps + checkpoint + a new Trainer resumed from it: the resumed state equals the saved one
    bit for bit, and the two final PSNRs agree within the native-vs-reference tolerance.  Measured on MI355X: 21.330 dB straight,
    21.322 dB resumed."""
    init, tb, vb, extent = load_scene(colmap_dir)
    conf = _gs_conf(1200, val_frequency=10 ** 9, validate_first=False, test_last=False, checkpoint=dict(iterations=[600]))
    straight = trainer_mod.Trainer(dict(conf, out_dir=str(tmp_path / "a")), init, tb, scene_extent=extent)
    straight.train()
    first = trainer_mod.Trainer(dict(conf, n_iterations=600, out_dir=str(tmp_path / "b")), init, tb, scene_extent=extent)
    first.train()
    path = str(tmp_path / "b" / "ours_600" / "ckpt_600.pt")
    saved = torch.load(path, weights_only=True)
    resumed = trainer_mod.Trainer(dict(conf, resume=path, out_dir=""), None, tb, scene_extent=extent)
    now = resumed.checkpoint()
    saved.pop("config"), now.pop("config")
    _equal(saved, now)
    assert resumed.global_step == 600 and resumed.model.n_active_features == saved["n_active_features"]
    resumed.train()
    a, b = evaluate(straight.model, straight.tracer, vb)["mean_psnr"], evaluate(resumed.model, resumed.tracer, vb)["mean_psnr"]
    print(f"\n[resume] psnr straight {a:.4f} resumed {b:.4f}, N {straight.model.num_gaussians} / {resumed.model.num_gaussians}")
    assert abs(a - b) <= PSNR_TOL


def test_cli_prints_statistics_and_test_metrics(colmap_dir, tmp_path):
    r = subprocess.run([sys.executable, "-m", "3dgrut_amd.trainer", "--path", colmap_dir, "--n-iterations", "200", "--out-dir", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    last = json.loads(r.stdout.strip().splitlines()[-1])
    assert last["stats"]["n_steps"] == 200 and last["stats"]["iteration_speed"] > 0
    assert last["test"]["n_views"] == 4 and last["test"]["mean_psnr"] > 0
