"""Pose-aligned held-out metrics without a GPU: the `pose_alignment` block, the aligner's host logic with an injected
step on a toy quadratic loss in the six pose coordinates, the option's path through the Trainer with a recording evaluator in the
style of tests/test_cpu_cc_metrics.py, and the C ABI surface of the pose-only backward."""
import ctypes as C
import importlib
import json
import types

import numpy as np
import pytest
import torch

from tests.test_cpu_pose_refiner import _views
from tests.test_cpu_trainer import _FakeStepper, _FakeStrategy, _model

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
pose_align = importlib.import_module("3dgrut_amd.pose_align")
pose_refine = importlib.import_module("3dgrut_amd.pose_refine")
pose = importlib.import_module("3dgrut_amd.pose")
capi = importlib.import_module("3dgrut_amd._capi")


# ---- the block ----
def test_defaults_pass_and_every_bad_value_is_named():
    assert pose_align.DEFAULTS == {"enabled": False, "validation": False, "iterations": 50, "lr_translation": 0.001, "lr_rotation": 0.0005,
                                   "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}
    assert pose_align.check_config(dict(pose_align.DEFAULTS)) == pose_align.DEFAULTS
    # the rates and the iteration count are the pose-refinement defaults' and the recovery test's
    for k in ("lr_translation", "lr_rotation", "beta1", "beta2", "eps"):
        assert pose_align.DEFAULTS[k] == pose_refine.DEFAULTS[k]
    bad = dict(enabled=["true", 1, None], validation=["false", 0], iterations=[-1, 2.5, "3", True, None],
               lr_translation=[-1e-3, float("nan"), float("inf"), "x", True], lr_rotation=[-1e-3, float("nan"), float("inf")],
               eps=[-1.0, float("nan"), float("inf")], beta1=[-0.1, 1.0, float("nan")], beta2=[1.0, 1.5, float("nan")])
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=f"pose_alignment.{key}"):
                pose_align.check_config(dict(pose_align.DEFAULTS, **{key: v}))
    with pytest.raises(ValueError, match="unknown keys.*iteration"):
        pose_align.check_config(dict(pose_align.DEFAULTS, iteration=3))
    assert pose_align.check_config(dict(pose_align.DEFAULTS, iterations=0))["iterations"] == 0
    conf = trainer_mod.resolve_config({})
    assert conf["evaluation"] == dict(colour_corrected=False, ridge=1e-6)      # the block lives at the top level, not in `evaluation`
    assert conf["pose_alignment"] == pose_align.DEFAULTS
    assert trainer_mod.default_config("MCMCStrategy")["pose_alignment"] == pose_align.DEFAULTS
    with pytest.raises(ValueError, match="pose_alignment.iterations"):
        trainer_mod.resolve_config(dict(pose_alignment=dict(iterations=-2)))
    with pytest.raises(ValueError, match="unknown"):
        trainer_mod.resolve_config(dict(pose_alignment=dict(lr=1e-3)))


# ---- the aligner's host logic ----
T_GIVEN = pose.apply_pose_increment(np.eye(4), [0.3, -0.2, -4.0, 0.02, -0.01, 0.03])
TARGET = np.array([0.31, -0.21, -3.98, 0.0, 0.0, 0.0])     # the camera centre the toy loss wants


class _QuadraticStep:
    """L(T) = 1/2 |c(T) - c*|^2 + 1/2 |phi(T)|^2 with phi the rotation vector of R(T) R_given^T: (loss, out8) with out8 = -(dL/d rho,
    dL/d phi) as the backward leaves it (dL/d rho = -F, dL/d phi = -M; for small phi the world-axis twist adds to phi).  Host tensors."""

    def __init__(self, losses=None):
        self.calls, self.poses, self.forced = 0, [], losses

    def __call__(self, batch):
        T = batch.T_to_world.reshape(4, 4).double().numpy()
        self.poses.append(T.copy())
        dr = T[:3, :3] @ T_GIVEN[:3, :3].T
        phi = 0.5 * np.array([dr[2, 1] - dr[1, 2], dr[0, 2] - dr[2, 0], dr[1, 0] - dr[0, 1]])
        g = np.concatenate([T[:3, 3] - TARGET[:3], phi])
        loss = 0.5 * float(g @ g)
        if self.forced is not None:
            loss = self.forced[self.calls]
        self.calls += 1
        out8 = torch.zeros(8)
        out8[:6] = torch.as_tensor(-g, dtype=torch.float32)
        return torch.tensor([loss], dtype=torch.float32), out8


def _batch(T=T_GIVEN, **extra):
    return types.SimpleNamespace(T_to_world=torch.as_tensor(T, dtype=torch.float32).reshape(1, 4, 4), **extra)


def test_iterates_are_the_host_adam_composed_by_apply_pose_increment():
    """K iterations: K + 1 losses, K + 1 poses visited; every T_{k+1} equals apply_pose_increment(T_k, delta_k) with delta_k from
    PoseRefiner's host-tensor Adam (one view, the same rates) fed the same gradients.  The batch handed to the step carries a
    float32 matrix; the aligner's own iterate stays float64, so the comparison is exact on the float32 images."""
    K = 12
    step = _QuadraticStep()
    res = pose_align.PoseAligner(step, iterations=K, lr_translation=5e-4, lr_rotation=5e-4).align(_batch())
    assert step.calls == K + 1 and len(res["losses"]) == K + 1
    ref = pose_refine.PoseRefiner([T_GIVEN.astype(np.float32)], "cpu", 5e-4, 5e-4)
    probe = _QuadraticStep()
    for k in range(K + 1):
        b = ref.begin(0, _batch())
        assert torch.equal(b.T_to_world.reshape(4, 4), torch.as_tensor(step.poses[k], dtype=torch.float32)), k
        if k < K:
            ref.end(0, probe(b)[1])
    assert res["losses"] == pytest.approx([0.5 * float(np.sum(np.square(probe_g))) for probe_g in _gradients(step.poses)], rel=1e-6)
    # the quadratic falls monotonically under these rates: the last iterate wins and the loss fell
    assert res["best_iteration"] == K and res["loss_aligned"] == res["losses"][K] < res["loss_given"] == res["losses"][0]
    assert np.array_equal(res["pose"], ref.poses[0]) and res["pose"].dtype == np.float64
    dt, dr = pose.pose_difference(res["pose"], T_GIVEN.astype(np.float32))
    assert res["translation"] == pytest.approx(dt) and res["rotation_deg"] == pytest.approx(np.degrees(dr))
    assert 0 < res["translation"] <= K * 5e-4 * np.sqrt(3) * 1.01           # Adam moves a coordinate by at most about one rate per step


def _gradients(poses):
    out = []
    for T in poses:
        dr = T[:3, :3] @ T_GIVEN[:3, :3].T
        phi = 0.5 * np.array([dr[2, 1] - dr[1, 2], dr[0, 2] - dr[2, 0], dr[1, 0] - dr[0, 1]])
        out.append(np.concatenate([T[:3, 3] - TARGET[:3], phi]))
    return out


def test_selection_smallest_index_wins_ties_and_non_finite_losses_never_win():
    al = lambda losses: pose_align.PoseAligner(_QuadraticStep(losses), iterations=len(losses) - 1).align(_batch())
    res = al([3.0, 2.0, 1.0, 1.0, 2.0])
    assert res["best_iteration"] == 2 and res["loss_aligned"] == 1.0 and res["loss_given"] == 3.0
    res = al([1.0, 1.0, 1.0])
    assert res["best_iteration"] == 0 and res["translation"] == 0.0 and res["rotation_deg"] == 0.0
    res = al([2.0, float("nan"), float("-inf"), 1.5, float("inf")])
    assert res["best_iteration"] == 3 and res["loss_aligned"] == 1.5
    res = al([float("nan"), 1.0, 0.5])                                     # l_0 not finite: the given pose
    assert res["best_iteration"] == 0 and np.array_equal(res["pose"], T_GIVEN.astype(np.float32).astype(np.float64))
    res = al([2.0, 3.0, 4.0])                                              # nothing better than the given pose
    assert res["best_iteration"] == 0 and res["loss_aligned"] == res["loss_given"] == 2.0
    for losses in ([3.0, 2.0, 1.0, 1.0, 2.0], [2.0, float("nan"), 5.0], [2.0, 3.0, 4.0]):
        r = al(losses)
        assert r["loss_aligned"] <= r["loss_given"]


def test_zero_iterations_return_the_given_matrix_bit_for_bit():
    T = torch.as_tensor(T_GIVEN, dtype=torch.float32).reshape(1, 4, 4)
    step = _QuadraticStep()
    res = pose_align.PoseAligner(step, iterations=0).align(types.SimpleNamespace(T_to_world=T))
    assert step.calls == 1 and len(res["losses"]) == 1 and res["best_iteration"] == 0
    assert res["pose"].dtype == np.float64 and np.array_equal(res["pose"], T.reshape(4, 4).double().numpy())
    assert torch.equal(torch.as_tensor(res["pose"], dtype=torch.float32), T.reshape(4, 4))
    assert res["translation"] == 0.0 and res["rotation_deg"] == 0.0 and res["loss_aligned"] == res["loss_given"]


def test_a_two_pose_batch_raises_before_the_step_is_called():
    step = _QuadraticStep()
    al = pose_align.PoseAligner(step, iterations=3)
    moved = pose.apply_pose_increment(T_GIVEN, [0.01, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="start and end poses differ"):
        al.align(_batch(T_to_world_end=torch.as_tensor(moved, dtype=torch.float32).reshape(1, 4, 4)))
    with pytest.raises(ValueError, match="ONE camera-to-world matrix"):
        al.align(types.SimpleNamespace(T_to_world=torch.stack([torch.eye(4), torch.eye(4)])))
    assert step.calls == 0
    al.align(_batch(T_to_world_end=torch.as_tensor(T_GIVEN, dtype=torch.float32).reshape(1, 4, 4)))   # equal poses: one pose
    assert step.calls == 4
    with pytest.raises(ValueError, match="iterations"):
        pose_align.PoseAligner(step, iterations=-1)


def test_the_step_is_bracketed_by_acquire_and_release_even_when_it_raises():
    class Step(_QuadraticStep):
        log = []

        def acquire(self):
            self.log.append("acquire")

        def release(self):
            self.log.append("release")

        def __call__(self, batch):
            if self.calls == 2:
                raise RuntimeError("boom")
            return super().__call__(batch)

    step = Step()
    with pytest.raises(RuntimeError, match="boom"):
        pose_align.PoseAligner(step, iterations=5).align(_batch())
    assert step.log == ["acquire", "release"]


# ---- the trainer ----
PA_RESULT = dict(mean_pa_psnr=24.0, std_pa_psnr=0.5, mean_pa_ssim=0.75, mean_pa_translation=0.0125, mean_pa_rotation_deg=0.25)


class _RecordingEvaluator:
    """Records how it was called; returns the pose-aligned keys only when asked for them, as evaluate() does."""

    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, dict(kwargs)))
        n = len(args[2])
        res = dict(mean_psnr=20.0, mean_ssim=0.5, std_psnr=0.25, psnr=[20.0] * n, ssim=[0.5] * n, n_views=n)
        if kwargs.get("colour_corrected"):
            res.update(mean_cc_psnr=23.0, std_cc_psnr=0.125, mean_cc_ssim=0.625)
        if kwargs.get("pose_aligned") is not None:
            res.update(PA_RESULT, pa_psnr=[24.0] * n, pa_poses=[np.eye(4).tolist()] * n)
            if kwargs.get("colour_corrected"):
                res.update(mean_pa_cc_psnr=25.0, std_pa_cc_psnr=0.0625, mean_pa_cc_ssim=0.875)
        return res


def _trainer(conf):
    conf = dict(conf, strategy=dict(method="GSStrategy"), out_dir="")
    ev = _RecordingEvaluator()
    tr = trainer_mod.Trainer(conf, None, _views(3), val_batches=_views(2), test_batches=_views(2), scene_extent=2.0,
                             stepper=_FakeStepper(_model()), strategy=_FakeStrategy(), evaluator=ev)
    return tr, ev


def test_option_off_calls_the_evaluator_as_before():
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2))
    res = tr.run()
    assert [kw for _, kw in ev.calls] == [{}, {}]
    assert set(tr.validations[0]) == {"step", "loss", "mean_psnr", "mean_ssim", "n_gaussians"}
    assert not any(k.startswith("mean_pa") for k in res["test"])
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2, evaluation=dict(colour_corrected=True)))
    tr.run()
    assert [kw for _, kw in ev.calls] == [dict(colour_corrected=True, ridge=1e-6)] * 2


def test_option_on_hands_over_resolved_settings_on_the_final_pass_only():
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2, pose_alignment=dict(enabled=True, iterations=7, lr_translation=0.003)))
    res = tr.run()
    assert len(ev.calls) == 2
    assert ev.calls[0][1] == {}                                            # the validation at step 2: off by default
    pa = ev.calls[1][1]["pose_aligned"]
    assert set(ev.calls[1][1]) == {"pose_aligned"}
    assert pa == dict(iterations=7, lr_translation=0.003 * 2.0, lr_rotation=0.0005, beta1=0.9, beta2=0.999, eps=1e-15,
                      lambda_l1=0.8, lambda_ssim=0.2)                      # times the scene extent; the run's loss weights
    assert "mean_pa_psnr" not in tr.validations[0]
    assert res["test"]["mean_pa_psnr"] == 24.0
    ck = tr.checkpoint()
    assert "pose_alignment" not in ck["native"] and ck["config"]["pose_alignment"]["enabled"] is True
    # validation: true -> the validation passes too, and their entries carry the means
    tr, ev = _trainer(dict(n_iterations=4, val_frequency=2, pose_alignment=dict(enabled=True, validation=True),
                           evaluation=dict(colour_corrected=True), loss=dict(lambda_l1=0.7, lambda_ssim=0.3)))
    tr.run()
    for _, kw in ev.calls:
        assert set(kw) == {"colour_corrected", "ridge", "pose_aligned"}
        assert kw["pose_aligned"]["lambda_l1"] == 0.7 and kw["pose_aligned"]["lambda_ssim"] == 0.3 and kw["pose_aligned"]["iterations"] == 50
    entry = tr.validations[0]
    assert {k: entry[k] for k in PA_RESULT} == PA_RESULT and entry["mean_pa_cc_psnr"] == 25.0 and entry["mean_cc_psnr"] == 23.0
    # validation: true alone switches nothing on
    tr, ev = _trainer(dict(n_iterations=2, val_frequency=1, pose_alignment=dict(validation=True)))
    tr.run()
    assert all(kw == {} for _, kw in ev.calls)


def test_command_line_switch():
    ap = trainer_mod.build_parser()
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--aligned-metrics"]))
    assert conf["pose_alignment"] == dict(pose_align.DEFAULTS, enabled=True)
    assert conf["pose_refinement"]["enabled"] is False and conf["evaluation"]["colour_corrected"] is False   # needs neither
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--aligned-metrics", "--align-iterations", "20", "--refine-poses",
                                                       "--exposure", "--cc-metrics"]))
    assert conf["pose_alignment"]["iterations"] == 20 and conf["pose_refinement"]["enabled"] and conf["evaluation"]["colour_corrected"]
    trainer_mod.resolve_config(conf)
    conf = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert conf["pose_alignment"] == pose_align.DEFAULTS
    with pytest.raises(ValueError, match="pose_alignment.iterations"):
        trainer_mod.resolve_config(trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--aligned-metrics", "--align-iterations", "-3"])))


def test_final_json_carries_the_aligned_means_only_when_present(monkeypatch, capsys):
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
    plain = dict(mean_psnr=20.0, std_psnr=0.25, mean_ssim=0.5, n_views=2)
    assert trainer_mod.main(["--path", "x", "--aligned-metrics"]) == 0
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last["test"] == dict(plain, **PA_RESULT)
    assert trainer_mod.main(["--path", "x", "--aligned-metrics", "--cc-metrics"]) == 0
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last["test"] == dict(plain, **PA_RESULT, mean_cc_psnr=23.0, std_cc_psnr=0.125, mean_cc_ssim=0.625, mean_pa_cc_psnr=25.0,
                                std_pa_cc_psnr=0.0625, mean_pa_cc_ssim=0.875)
    assert trainer_mod.main(["--path", "x"]) == 0
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last["test"] == plain


# ---- the C ABI ----
def test_the_pose_only_backward_is_exported_with_its_declared_arguments():
    lib = capi.load()
    assert "gut_trace_bwd_pose" in capi.EXPORTS and hasattr(lib, "gut_trace_bwd_pose")
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    # gut_trace_bwd_ex's arguments without the radiance rows, the two gradient outputs and the flags
    assert lib.gut_trace_bwd_pose.argtypes == [vp, vp, u32, i32, u32, vp, i32, i32, vp, vp, C.POINTER(capi.GutCamera), vp, vp, vp, vp]
    assert lib.gut_abi_version() == 6 == capi.GUT_ABI_VERSION            # added without a bump
    # refused on the host: a null handle returns 1 on a machine without a GPU
    cam = capi.GutCamera()
    assert lib.gut_trace_bwd_pose(None, None, 0, 3, 0, None, 64, 64, None, None, C.byref(cam), None, None, None, None) == 1
    assert b"gut_trace_bwd_pose: null handle" in lib.gut_last_error()
    tracer_mod = importlib.import_module("3dgrut_amd.tracer")
    assert callable(tracer_mod.SplatRaster.trace_bwd_pose)
