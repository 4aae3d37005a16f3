"""The trainer with --refine-poses on a small synthetic COLMAP scene: the command-line run finishes and reports how far the poses
moved, and a Trainer resumed from its checkpoint continues from the same poses."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.synthetic_colmap import load_scene, write_synthetic_colmap

pytestmark = pytest.mark.gpu
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_run_refines_the_poses_and_a_resume_continues_from_them(tmp_path):
    scene = write_synthetic_colmap(str(tmp_path / "scene"), n_views=16, size=160, n_teacher=40_000, n_points=4_000)
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, "-m", "3dgrut_amd.trainer", "--path", scene, "--n-iterations", "60", "--out-dir", out,
                        "--refine-poses", "--pose-lr-rotation", "0.0004"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    assert last["stats"]["n_steps"] == 60 and last["test"]["mean_psnr"] > 0
    assert last["stats"]["pose_mean_translation"] > 0 and last["stats"]["pose_mean_rotation_deg"] > 0

    path = os.path.join(out, "ckpt_last.pt")
    saved = torch.load(path, weights_only=True)["native"]["pose_refinement"]
    init, tb, vb, extent = load_scene(scene)
    given = torch.stack([b.T_to_world.detach().cpu().to(torch.float64).reshape(4, 4) for b in tb])
    assert tuple(saved["poses"].shape) == (len(tb), 4, 4) and saved["poses"].dtype == torch.float64
    assert torch.allclose(saved["initial_poses"], given, rtol=0, atol=1e-6)
    assert int(saved["counts"].sum()) == 60
    moved = (saved["poses"] - given).abs().amax((1, 2))
    assert bool((moved[saved["counts"] > 0] > 0).all())
    # held-out views keep their given poses: nothing of the refiner refers to them
    conf = trainer_mod.default_config("GSStrategy")
    conf.update(n_iterations=64, resume=path, out_dir="", test_last=False, val_frequency=10 ** 9)
    conf["pose_refinement"].update(enabled=True, lr_rotation=0.0004)
    tr = trainer_mod.Trainer(conf, None, tb, val_batches=vb, scene_extent=extent)
    assert tr.global_step == 60
    assert torch.equal(tr.refined_poses(), saved["poses"]) and not torch.equal(tr.refined_poses(), given)
    assert torch.equal(tr.refiner.counts.cpu(), saved["counts"]) and torch.equal(tr.refiner.m.cpu(), saved["exp_avg"])
    seen = []
    step = tr.stepper.step
    tr.stepper.step = lambda b: (seen.append(b.T_to_world.clone()), step(b))[1]
    tr.train()
    view = tr.batch_index(60)
    assert torch.equal(seen[0][0], saved["poses"][view].to(torch.float32))     # the first resumed step renders the saved pose
    assert tr.global_step == 64 and int(tr.refiner.counts.sum()) == 64
    assert torch.isfinite(tr.model.raw).all() and torch.isfinite(tr.refined_poses()).all()
