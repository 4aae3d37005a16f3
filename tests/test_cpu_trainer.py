"""The end-to-end Trainer without a GPU: loop order (validation, checkpoints, strategy calls, epochs, resume) with a fake stepper,
strategy and evaluator, the checkpoint layout (reference keys, torch.optim.Adam state-dict form, exact round trip, weights_only),
and the SSIM equivalence the evaluation metric rests on."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
native = importlib.import_module("3dgrut_amd.native")
scenes = importlib.import_module("3dgrut_amd.scenes")
train = importlib.import_module("3dgrut_amd.train")
Batch = importlib.import_module("3dgrut_amd.protocols").Batch


def _batch(tag, mask=False, gt=True):
    z = torch.zeros((1, 12, 12, 3))
    b = Batch(rays_ori=z, rays_dir=z, T_to_world=torch.eye(4)[None], rgb_gt=z.clone() if gt else None,
              mask=torch.ones((1, 12, 12, 1)) if mask else None)
    b.tag = tag
    return b


class _FakeStepper:
    """NativeTrainStep's surface as the Trainer uses it, on CPU tensors: step() records (step, view) and halves the position
    learning rate (a stand-in for the schedule that runs at the end of the real step)."""

    def __init__(self, model, seed=0):
        g = torch.Generator().manual_seed(seed)
        n = model.num_gaussians
        self.model = model
        self.m12, self.v12 = torch.randn((n, 12), generator=g), torch.rand((n, 12), generator=g)
        self.m48, self.v48 = torch.randn((n, 48), generator=g), torch.rand((n, 48), generator=g)
        self.lr12 = np.linspace(1e-4, 1e-2, 12).astype(np.float32)
        self.lr48 = np.linspace(1e-5, 1e-3, 48).astype(np.float32)
        self.betas, self.eps, self.schedule = (0.9, 0.999), 1e-15, None
        self.step_id = 0
        self.steps = []

    def step(self, batch):
        self.steps.append((self.step_id, batch.tag))
        self.step_id += 1
        self.lr12[0:3] *= 0.5
        return torch.tensor(0.25), {}

    def state_dict(self):
        return dict(step=self.step_id, exp_avg_raw=self.m12.clone(), exp_avg_sq_raw=self.v12.clone(), exp_avg_features=self.m48.clone(),
                    exp_avg_sq_features=self.v48.clone(), lr_raw=self.lr12.copy())


class _FakeStrategy:
    def __init__(self):
        self.calls = []

    def post_optimizer_step(self, step, arg):
        self.calls.append((step, arg))


class _FakeEvaluator:
    def __init__(self):
        self.steps = []

    def __call__(self, model, tracer, batches, out_dir, step):
        self.steps.append(step)
        return dict(mean_psnr=20.0, mean_ssim=0.5, std_psnr=0.0, psnr=[20.0] * len(batches), ssim=[0.5] * len(batches))


def _model(n=37, seed=2):
    sc = scenes.scene_c1(n, seed)
    m = native.NativeGaussianModel(sc, device="cpu")
    m.raw[:, 11] = torch.arange(n, dtype=torch.float32)   # the unused pad column: must survive a round trip too
    return m


def _trainer(conf, views=3, method="GSStrategy", stepper=None):
    conf = dict(conf, strategy=dict(method=method))
    st = stepper or _FakeStepper(_model())
    strat, ev = _FakeStrategy(), _FakeEvaluator()
    tr = trainer_mod.Trainer(conf, None, [_batch(i) for i in range(views)], val_batches=[_batch(100)], scene_extent=2.5, stepper=st,
                             strategy=strat, evaluator=ev)
    saved = []
    tr.save_checkpoint = lambda last=False: saved.append(tr.global_step)
    return tr, st, strat, ev, saved


@pytest.mark.parametrize("validate_first", [False, True])
def test_loop_order_validation_checkpoints_and_epochs(validate_first):
    """trainer.py:705-806 for n_iterations = 7 over 3 views: validation before the step when (g > 0 or validate_first) and
    g % val_frequency == 0, checkpoints after the increment (post-increment step in checkpoint.iterations), the strategy called
    with (g, scene_extent) after every step, and the step count held across epochs."""
    tr, st, strat, ev, saved = _trainer(dict(n_iterations=7, val_frequency=3, validate_first=validate_first,
                                             checkpoint=dict(iterations=[2, 5, 7, 9])))
    stats = tr.train()
    assert stats["n_steps"] == 7 and tr.global_step == 7 and len(st.steps) == 7
    assert ev.steps == ([0, 3, 6] if validate_first else [3, 6])
    assert saved == [2, 5, 7]
    assert strat.calls == [(g, 2.5) for g in range(7)]
    assert [s for s, _ in st.steps] == list(range(7))
    views = [v for _, v in st.steps]
    for e in range(3):   # every epoch is a permutation of the views, drawn from (seed, epoch)
        perm = trainer_mod.epoch_permutation(0, e, 3)
        assert sorted(perm) == [0, 1, 2]
        assert views[3 * e:3 * e + 3] == perm[:len(views[3 * e:3 * e + 3])]
    assert stats["iteration_speed"] > 0 and stats["training_time"] > 0
    assert [v["step"] for v in tr.validations] == ev.steps and tr.validations[-1]["loss"] == 0.25


def test_mcmc_post_optimizer_step_gets_the_scheduled_position_lr():
    """MCMC: post_optimizer_step(g, current position lr) — the rate after the step's own scheduler update (trainer.py:756-762)."""
    tr, st, strat, _, _ = _trainer(dict(n_iterations=4, val_frequency=1000), method="MCMCStrategy")
    lr0 = float(st.lr12[0])
    tr.train()
    assert [g for g, _ in strat.calls] == [0, 1, 2, 3]
    for g, lr in strat.calls:
        assert lr == pytest.approx(lr0 * 0.5 ** (g + 1), rel=1e-6)


def test_resume_mid_epoch_continues_the_view_order(tmp_path):
    """A run resumed at step 4 of 3-view epochs (mid-epoch) takes the same views in steps 4.. as an uninterrupted run."""
    full, st_full, _, _, _ = _trainer(dict(n_iterations=10, val_frequency=1000), views=3)
    full.train()
    part, st_part, _, _, _ = _trainer(dict(n_iterations=4, val_frequency=1000), views=3)
    part.train()
    path = tmp_path / "ckpt_4.pt"
    torch.save(part.checkpoint(), path)
    resumed, st_res, _, _, _ = _trainer(dict(n_iterations=10, val_frequency=1000, resume=str(path)), views=3)
    assert resumed.global_step == 4 and resumed.epoch == 1
    resumed.train()
    assert [v for _, v in st_part.steps] == [v for _, v in st_full.steps][:4]
    assert [v for _, v in st_res.steps] == [v for _, v in st_full.steps][4:]


def test_masked_or_unlabelled_batches_are_refused():
    st = _FakeStepper(_model())
    with pytest.raises(ValueError, match="mask"):
        trainer_mod.Trainer({}, None, [_batch(0), _batch(1, mask=True)], stepper=st, strategy=_FakeStrategy())
    with pytest.raises(ValueError, match="rgb_gt"):
        trainer_mod.Trainer({}, None, [_batch(0)], test_batches=[_batch(1, gt=False)], stepper=st, strategy=_FakeStrategy())


def test_checkpoint_layout_adam_state_and_exact_round_trip(tmp_path):
    """Reference keys (model.py:107-134) with their shapes, torch.optim.Adam's state-dict form (a CPU Adam over six parameters of
    those shapes loads it, exp_avg = the native moment columns), GS buffers as 1-tuples, weights_only loading, and native state ->
    checkpoint -> native state bit for bit."""
    m = _model(41)
    st = _FakeStepper(m, seed=4)
    st.step_id = 123
    gs = _FakeStrategy()
    gs.grad_norm_accum = torch.rand((41, 1))
    gs.grad_norm_denom = torch.randint(0, 9, (41, 1), dtype=torch.int32)
    conf = trainer_mod.resolve_config({})
    ck = trainer_mod.make_checkpoint(st, conf, global_step=123, epoch=3, scene_extent=2.5, strategy=gs)
    n = 41
    shapes = dict(positions=(n, 3), rotation=(n, 4), scale=(n, 3), density=(n, 1), features_albedo=(n, 3), features_specular=(n, 45))
    for k, s in shapes.items():
        assert tuple(ck[k].shape) == s, k
    for k in ("background", "n_active_features", "max_n_features", "progressive_training", "scene_extent", "optimizer", "config",
              "feature_dim_increase_interval", "feature_dim_increase_step", "global_step", "epoch", "native"):
        assert k in ck, k
    assert tuple(ck["background"]["color"].shape) == (3,)
    assert ck["global_step"] == 123 and ck["epoch"] == 3 and ck["scene_extent"] == 2.5 and ck["max_n_features"] == 3
    assert isinstance(ck["densify_grad_norm_accum"], tuple) and torch.equal(ck["densify_grad_norm_accum"][0], gs.grad_norm_accum)
    assert torch.equal(ck["densify_grad_norm_denom"][0], gs.grad_norm_denom)

    path = tmp_path / "ckpt.pt"
    torch.save(ck, path)
    ck = torch.load(path, weights_only=True)

    params = [torch.nn.Parameter(torch.zeros(shapes[name])) for name in trainer_mod.PARAM_GROUPS]
    opt = torch.optim.Adam([dict(params=[p], lr=1.0, name=name) for p, name in zip(params, trainer_mod.PARAM_GROUPS)], eps=1e-15)
    opt.load_state_dict(ck["optimizer"])
    assert [g["name"] for g in opt.param_groups] == list(trainer_mod.PARAM_GROUPS)
    cols = dict(positions=st.m12[:, 0:3], density=st.m12[:, 3:4], rotation=st.m12[:, 4:8], scale=st.m12[:, 8:11],
                features_albedo=st.m48[:, 0:3], features_specular=st.m48[:, 3:])
    for p, name in zip(params, trainer_mod.PARAM_GROUPS):
        assert torch.equal(opt.state[p]["exp_avg"], cols[name]), name
        assert float(opt.state[p]["step"]) == 123.0
    assert opt.param_groups[0]["lr"] == pytest.approx(float(st.lr12[0]))
    opt.step()   # the loaded state is usable

    raw, features, state = trainer_mod.checkpoint_tensors(ck, "cpu")
    assert torch.equal(raw, m.raw) and torch.equal(features, m.features)
    for key, ref in (("exp_avg_raw", st.m12), ("exp_avg_sq_raw", st.v12), ("exp_avg_features", st.m48), ("exp_avg_sq_features", st.v48)):
        assert torch.equal(state[key], ref), key
    assert state["step"] == 123 and np.array_equal(state["lr_raw"], st.lr12)


def _torchmetrics_ssim(x, y, k=11, sigma=1.5, c1=0.01 ** 2, c2=0.03 ** 2):
    """StructuralSimilarityIndexMeasure(data_range=1)'s procedure: reflect-pad by the window radius, filter, clamp the two variances
    at 0, then crop exactly the padded border before the mean."""
    c, pad = x.shape[1], (k - 1) // 2
    g = train._gauss_window(k, sigma, dtype=x.dtype)
    kern = (g[:, None] * g[None, :]).expand(c, 1, k, k)
    xp, yp = F.pad(x, (pad,) * 4, mode="reflect"), F.pad(y, (pad,) * 4, mode="reflect")
    blur = lambda t: F.conv2d(t, kern, groups=c)
    mu_x, mu_y = blur(xp), blur(yp)
    sxx = torch.clamp(blur(xp * xp) - mu_x ** 2, min=0.0)
    syy = torch.clamp(blur(yp * yp) - mu_y ** 2, min=0.0)
    sxy = blur(xp * yp) - mu_x * mu_y
    m = ((2 * mu_x * mu_y + c1) * (2 * sxy + c2)) / ((mu_x ** 2 + mu_y ** 2 + c1) * (sxx + syy + c2))
    return m[..., pad:-pad, pad:-pad].mean()


@pytest.mark.parametrize("hw", [(11, 11), (37, 129), (64, 48)])
def test_torchmetrics_ssim_equals_the_valid_region_training_ssim(hw):
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    x = torch.rand((1, 3) + hw, generator=g, dtype=torch.float64)
    y = (x + 0.2 * torch.randn(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    ref = train.ssim(x, y, window=train._gauss_window(dtype=torch.float64))
    assert abs(float(_torchmetrics_ssim(x, y)) - float(ref)) <= 1e-12
