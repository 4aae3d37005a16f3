"""PoseRefiner and its place in the Trainer without a GPU: per-view Adam bookkeeping, the deferred increment, the checkpoint round
trip and the config validation, with a fake stepper in the style of tests/test_cpu_trainer.py."""
import importlib

import numpy as np
import pytest
import torch

from tests.common import cams
from tests.test_cpu_trainer import _FakeEvaluator, _FakeStepper, _FakeStrategy, _model

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
native = importlib.import_module("3dgrut_amd.native")
pose = importlib.import_module("3dgrut_amd.pose")
pose_refine = importlib.import_module("3dgrut_amd.pose_refine")
Batch = importlib.import_module("3dgrut_amd.protocols").Batch


def _views(n):
    z = torch.zeros((1, 12, 12, 3))
    out = []
    for i in range(n):
        b = Batch(rays_ori=z, rays_dir=z, T_to_world=torch.as_tensor(cams.orbit_c2w(4.0, 40.0 * i, 10.0))[None], rgb_gt=z.clone())
        b.tag = i
        out.append(b)
    return out


def _refiner(n=3, **kw):
    views = _views(n)
    args = dict(lr_translation=1e-3, lr_rotation=5e-4)
    args.update(kw)
    return pose_refine.PoseRefiner([b.T_to_world for b in views], "cpu", **args), views


def _grad8(seed):
    g = torch.zeros(8)
    g[:6] = torch.as_tensor(np.random.default_rng(seed).standard_normal(6), dtype=torch.float32)
    g[6] = 17.0
    return g


def test_moments_and_counts_advance_only_for_the_visited_view():
    r, views = _refiner(3)
    g = _grad8(0)
    r.begin(1, views[1])
    r.end(1, g)
    assert r.counts.tolist() == [0, 1, 0]
    assert not r.m[0].any() and not r.m[2].any() and not r.v[0].any() and not r.v[2].any()
    # Adam's first step from zero moments: m = (1 - b1) g, v = (1 - b2) g^2, bias-corrected by the view's OWN count (1), so the
    # increment is -lr * sign(g) up to eps — and g is (-F, -M)
    assert torch.allclose(r.m[1], -0.1 * g[:6], rtol=1e-6, atol=0)
    assert torch.allclose(r.v[1], 0.001 * g[:6] ** 2, rtol=1e-4, atol=0)   # (1 - beta2 is held in float32: 0.0010000467)
    lr = torch.tensor([1e-3] * 3 + [5e-4] * 3)
    assert torch.allclose(r._slots[1], lr * torch.sign(g[:6]), rtol=1e-5, atol=0)
    # a second visit of ANOTHER view starts its own count at 1: the same first-step increment, not a step-2 one
    r.begin(2, views[2])
    r.end(2, g)
    assert r.counts.tolist() == [0, 1, 1]
    assert torch.equal(r._slots[2], r._slots[1]) and torch.equal(r.m[2], r.m[1])
    # and the second visit of view 1 uses count 2
    r.begin(1, views[1])
    r.end(1, g)
    assert r.counts.tolist() == [0, 2, 1]
    m2 = 0.9 * (-0.1 * g[:6]) + 0.1 * -g[:6]
    assert torch.allclose(r.m[1], m2, rtol=1e-5, atol=0)


def test_a_pending_increment_is_applied_exactly_once_at_the_views_next_begin():
    r, views = _refiner(2)
    p0 = r.poses.copy()
    out = r.begin(0, views[0])
    assert out is not views[0] and out.tag == 0 and out.rays_dir is views[0].rays_dir      # rays stay as they are
    assert not out.T_to_world.is_cuda and out.T_to_world.dtype == torch.float32 and tuple(out.T_to_world.shape) == (1, 4, 4)
    assert torch.equal(out.T_to_world[0], views[0].T_to_world[0])                          # nothing pending: the given pose
    assert torch.equal(views[0].T_to_world[0], torch.as_tensor(cams.orbit_c2w(4.0, 0.0, 10.0)))   # the caller's batch is untouched
    r.end(0, _grad8(3))
    assert np.array_equal(r.poses, p0)                    # not applied yet ...
    r.begin(1, views[1])
    assert np.array_equal(r.poses, p0)                    # ... nor by another view's begin
    with pytest.raises(RuntimeError, match="no begin"):
        r.end(0, _grad8(4))                               # two end() without a begin() would lose an increment
    delta = r._slots[0].numpy().astype(np.float64)
    expect = pose.apply_pose_increment(p0[0], delta)
    out = r.begin(0, views[0])
    assert np.array_equal(r.poses[0], expect) and np.array_equal(r.poses[1], p0[1])
    assert torch.equal(out.T_to_world[0], torch.as_tensor(expect, dtype=torch.float32))
    again = r.begin(0, views[0])                          # no second application
    assert np.array_equal(r.poses[0], expect) and torch.equal(again.T_to_world, out.T_to_world)
    assert np.abs(r.poses[0][:3, 3] - p0[0][:3, 3]).max() == pytest.approx(1e-3, rel=1e-4)
    ch = r.pose_change()
    assert ch["mean_translation"] == pytest.approx(0.5 * np.sqrt(3) * 1e-3, rel=1e-3) and ch["mean_rotation_deg"] > 0


def test_window_of_iterations():
    r, _ = _refiner(2, start_iteration=5, end_iteration=9)
    assert [g for g in range(12) if r.active(g)] == [5, 6, 7, 8]
    r, _ = _refiner(2, start_iteration=2)
    assert not r.active(1) and r.active(2) and r.active(10 ** 9)


class _PoseStepper(_FakeStepper):
    """The fake stepper with NativeTrainStep(pose_gradient=True)'s surface: step() leaves a gradient that depends on the view."""
    world_size = 1

    def __init__(self, model, seed=0):
        super().__init__(model, seed)
        self.pose_gradient = torch.zeros(8)
        self.poses_seen = []
        self.switched = []

    def enable_pose_gradient(self, on):
        self.switched.append(bool(on))

    def step(self, batch):
        self.poses_seen.append((batch.tag, batch.T_to_world.clone()))
        self.pose_gradient.copy_(_grad8(100 + batch.tag))
        return super().step(batch)


def _trainer(conf, views=3, stepper=None):
    conf = dict(conf, strategy=dict(method="GSStrategy"))
    st = stepper or _PoseStepper(_model())
    return trainer_mod.Trainer(conf, None, _views(views), val_batches=_views(1), scene_extent=2.0, stepper=st, strategy=_FakeStrategy(),
                               evaluator=_FakeEvaluator()), st


def test_option_is_off_by_default_and_validated():
    conf = trainer_mod.resolve_config({})
    assert conf["pose_refinement"] == pose_refine.DEFAULTS and conf["pose_refinement"]["enabled"] is False
    tr, st = _trainer(dict(n_iterations=4, val_frequency=1000), stepper=_FakeStepper(_model()))
    assert tr.refiner is None
    tr.train()
    given = torch.stack([b.T_to_world[0].to(torch.float64) for b in tr.train_batches])
    assert torch.equal(tr.refined_poses(), given) and "pose_mean_translation" not in tr.stats
    assert "pose_refinement" not in tr.checkpoint()["native"]
    with pytest.raises(ValueError, match="beta1"):
        trainer_mod.resolve_config(dict(pose_refinement=dict(beta1=1.0)))
    with pytest.raises(ValueError, match="lr_rotation"):
        trainer_mod.resolve_config(dict(pose_refinement=dict(lr_rotation=-1.0)))
    with pytest.raises(ValueError, match="unknown"):
        trainer_mod.resolve_config(dict(pose_refinement=dict(learning_rate=1.0)))
    with pytest.raises(ValueError, match="enabled"):
        trainer_mod.resolve_config(dict(pose_refinement=dict(enabled="false")))
    for bad in (dict(start_iteration=1.5), dict(end_iteration="10"), dict(start_iteration=-1), dict(end_iteration=-2), dict(start_iteration=True)):
        with pytest.raises(ValueError, match="iteration"):
            trainer_mod.resolve_config(dict(pose_refinement=bad))
    r, views = _refiner(2)
    with pytest.raises(ValueError, match="the gradient is on"):
        r.end(0, torch.zeros(8, device="meta"))
    # a stepper that leaves no pose gradient cannot refine; nor can a data-parallel one
    with pytest.raises(ValueError, match="pose gradient"):
        _trainer(dict(pose_refinement=dict(enabled=True)), stepper=_FakeStepper(_model()))
    dp = _PoseStepper(_model())
    dp.world_size = 2
    with pytest.raises(ValueError, match="world_size"):
        _trainer(dict(pose_refinement=dict(enabled=True)), stepper=dp)
    with pytest.raises(ValueError, match="world_size"):
        native.NativeTrainStep(None, None, world_size=2, pose_gradient=True)


def test_trainer_loop_refines_each_view_from_its_own_gradients_and_resumes_bit_for_bit(tmp_path):
    conf = dict(n_iterations=7, val_frequency=1000, pose_refinement=dict(enabled=True, lr_translation=1e-3, lr_rotation=5e-4,
                                                                        start_iteration=1))
    tr, st = _trainer(conf)
    assert tr.refiner.lr_translation == pytest.approx(2e-3)       # times the scene extent
    tr.train()
    assert st.switched == [False] + [True] * 6                    # the output is off outside [start_iteration, end_iteration)
    order = [v for v, _ in st.poses_seen]
    # step 0 is before start_iteration: no update from it; every later visit counts for its own view
    visits = {v: sum(1 for g, w in enumerate(order) if w == v and g >= 1) for v in range(3)}
    assert tr.refiner.counts.tolist() == [visits[v] for v in range(3)]
    # the stepper saw, at every visit, the given pose composed with the increments of that view's EARLIER visits only
    first = {}
    for g, (v, T) in enumerate(st.poses_seen):
        if v not in first:
            first[v] = g
            assert torch.equal(T, tr.train_batches[v].T_to_world), (g, v)
    assert any(not torch.equal(T, tr.train_batches[v].T_to_world) for v, T in st.poses_seen)
    poses = tr.refined_poses()
    assert poses.dtype == torch.float64 and tuple(poses.shape) == (3, 4, 4)
    assert tr.stats["pose_mean_translation"] > 0 and tr.stats["pose_mean_rotation_deg"] > 0
    assert tr.refiner._pending == [False, False, False]

    ck = tr.checkpoint()
    path = tmp_path / "ckpt.pt"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=True)            # tensors only under `native`
    saved = ck["native"]["pose_refinement"]
    assert all(isinstance(x, torch.Tensor) for x in saved.values())
    with pytest.raises(ValueError, match="holds refined poses"):    # a resume must not silently fall back to the given poses
        _trainer(dict(n_iterations=9, val_frequency=1000, resume=str(path)))
    tr2, st2 = _trainer(dict(conf, n_iterations=9, resume=str(path)))
    assert tr2.global_step == 7
    for a, b in ((tr2.refiner.poses, tr.refiner.poses), (tr2.refiner.initial, tr.refiner.initial)):
        assert a.tobytes() == b.tobytes()
    assert torch.equal(tr2.refiner.m, tr.refiner.m) and torch.equal(tr2.refiner.v, tr.refiner.v)
    assert torch.equal(tr2.refiner.counts, tr.refiner.counts)
    # the resumed run continues from the same poses: its first step renders view 7's pose as the uninterrupted run would
    tr3, st3 = _trainer(dict(conf, n_iterations=9))
    tr3.train()
    tr2.train()
    assert [v for v, _ in st2.poses_seen] == [v for v, _ in st3.poses_seen][7:]
    for (_, a), (_, b) in zip(st2.poses_seen, st3.poses_seen[7:]):
        assert torch.equal(a, b)
    assert torch.equal(tr2.refined_poses(), tr3.refined_poses())
