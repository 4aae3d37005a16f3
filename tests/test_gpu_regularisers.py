"""The MCMC recipe's opacity / scale regularisers (configs/base_mcmc.yaml:13-18, trainer.py:432-449) in the native train step:
against the autograd step with the same loss, against torch.optim.Adam on the closed-form gradient, across the optimiser's
one- / two-pass, lazy / eager, exchange and selective forms, and in an MCMC run on the live trainer."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests.common import cams, make_view, rel_l2, scenes, to_batch

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
native = importlib.import_module("3dgrut_amd.native")
train = importlib.import_module("3dgrut_amd.train")
losses = importlib.import_module("3dgrut_amd.losses")
strategy = importlib.import_module("3dgrut_amd.strategy")
model_mod = importlib.import_module("3dgrut_amd.model")
DEV = "cuda:0"


def _batch(view, gt, host_pose=False):
    b = to_batch(view, DEV)
    if host_pose:
        b.T_to_world = b.T_to_world.cpu()
    b.rgb_gt = gt
    return b


def _state(st):
    return dict(raw=st.model.raw, features=st.model.features, m12=st.m12, v12=st.v12, m48=st.m48, v48=st.v48, act=st.act)


def _torch_reg(raw, lo, ls):
    """(opacity_loss, scale_loss) of raw [N,12] rows in float64: losses.regularisation_loss on the activations."""
    r = raw.double()
    return losses.regularisation_loss(torch.sigmoid(r[:, 3:4]), torch.exp(r[:, 8:11]), lo, ls)


def _rows_in_unwalked_waves(raster, n):
    """Boolean [n]: rows of 64-row waves that hold no Gaussian among the list entries the forward walked."""
    ranges = raster.debug_buffer("tile_ranges").view(-1, 2).long()
    trav = torch.minimum(raster.debug_buffer("tile_traversed_fwd").long(), ranges[:, 1] - ranges[:, 0])
    ids = raster.debug_buffer("ordered_ids").long()
    total = int(trav.sum())
    tile_of = torch.repeat_interleave(torch.arange(trav.numel(), device=ids.device), trav)
    off = torch.arange(total, device=ids.device) - torch.repeat_interleave(torch.cumsum(trav, 0) - trav, trav)
    walked_ids = ids[ranges[:, 0][tile_of] + off]
    walked_ids = walked_ids[(walked_ids >= 0) & (walked_ids < n)]
    waves = torch.zeros((n + 63) // 64, dtype=torch.bool, device=ids.device)
    waves[walked_ids // 64] = True
    return ~waves.repeat_interleave(64)[:n]


def _gradient_free_waves(raster, n):
    """Boolean [n]: rows of the waves that cannot receive a photometric gradient (no tile in the wave, or nothing of it walked)."""
    cnt = raster.debug_buffer("tiles_count")
    pad = (-n) % 64
    has = torch.nn.functional.pad(cnt != 0, (0, pad)).view(-1, 64).any(1)
    unw = torch.nn.functional.pad(_rows_in_unwalked_waves(raster, n), (0, pad), value=True).view(-1, 64).all(1)
    return ((~has) | unw).repeat_interleave(64)[:n]


# ---- 1. native vs autograd with the MCMC loss ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.01, 1.0])
@pytest.mark.parametrize("mode", ["dense", "compact", "one_pass"])
@pytest.mark.parametrize("steps", [1, 3])
def test_regularised_native_step_matches_autograd_step(steps, mode, lam):
    sc = scenes.scene_c1(800, 21)
    view = make_view("pinhole", 96, 80, cams.look_at_c2w((0.2, -0.1, -3.5), (0, 0, 0)), fx=90)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, 80, 96, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    ma = model_mod.GaussianModel(sc, device=DEV)
    ta = train.TrainStep(ma, gut.Tracer({"render": {}}), scene_extent=1.0, lambda_opacity=lam, lambda_scale=lam)
    mn = native.NativeGaussianModel(sc, device=DEV)
    tn = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0, fused_sh_adam=mode != "dense",
                                fuse_epilogue=(mode == "one_pass"), lambda_opacity=lam, lambda_scale=lam)
    for _ in range(steps):
        with torch.no_grad():
            ref_o, ref_s = _torch_reg(mn.raw, lam, lam)
        la, oa = ta.step(batch)
        ln, on = tn.step(batch)
        assert abs(float(la) - float(ln)) <= 1e-5
        for key, ref in (("opacity_loss", ref_o), ("scale_loss", ref_s)):
            assert on[key].is_cuda and on[key].dim() == 0
            assert abs(float(on[key]) - float(ref)) <= 1e-6 * abs(float(ref)), key
            assert abs(float(oa[key]) - float(ref)) <= 1e-6 * abs(float(ref)), key
    raw = mn.raw.cpu().numpy()
    tol = 2e-5 if steps == 1 else 2e-4
    assert rel_l2(raw[:, 0:3], ma.positions.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 3:4], ma.density.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 4:8], ma.rotation.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 8:11], ma.scale.detach().cpu().numpy()) <= tol
    feats = torch.cat([ma.features_albedo, ma.features_specular], 1).detach().cpu().numpy()
    assert rel_l2(mn.features.cpu().numpy(), feats) <= tol


# ---- 2. unseen Gaussians follow Adam on the regulariser alone ------------------------------------------------------------------
def test_unseen_gaussians_follow_adam_on_the_regulariser_alone():
    sc = scenes.scene_c1(3000, 7)
    hidden = slice(3000 - 640, 3000)   # ten whole 64-row waves
    sc["positions"][hidden] = sc["positions"][hidden] * 0.5 + np.array([0.0, 0.0, -9.0])   # behind the camera: never a tile
    view = make_view("pinhole", 96, 72, cams.look_at_c2w((0.0, 0.0, -4.0), (0, 0, 0)), fx=90)
    gt = torch.rand((1, 72, 96, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    lo, ls = 0.01, 0.01
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True, lazy_moments=True,
                                lambda_opacity=lo, lambda_scale=ls)
    assert st.lazy_moments
    n = model.num_gaussians
    raw0, feat0 = model.raw[hidden].clone(), model.features[hidden].clone()
    # the reference: float32 torch.optim.Adam, the reference's column groups and rates, the closed-form gradient
    groups = [(slice(0, 3), float(st.lr12[0])), (slice(3, 4), float(st.lr12[3])), (slice(4, 8), float(st.lr12[4])),
              (slice(8, 11), float(st.lr12[8]))]
    params = [torch.nn.Parameter(raw0[:, c].clone()) for c, _ in groups]
    # (the float32 betas the kernels use: 1 - 0.999f is 0.00099998713, 1.3e-5 away from the 0.001 torch forms from a Python 0.999)
    betas32 = tuple(float(np.float32(b)) for b in st.betas)
    opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, (_, lr) in zip(params, groups)], betas=betas32, eps=st.eps)
    for _ in range(20):
        st.step(_batch(view, gt, host_pose=True))
        assert int(st.raster.debug_buffer("tiles_count")[hidden].abs().sum()) == 0
        with torch.no_grad():
            sig = torch.sigmoid(params[1])
            params[0].grad = torch.zeros_like(params[0])
            params[1].grad = (lo / n) * sig * (1 - sig)
            params[2].grad = torch.zeros_like(params[2])
            params[3].grad = (ls / (3 * n)) * torch.exp(params[3])
        opt.step()
    got = model.raw[hidden]
    for p, (c, _) in zip(params, groups):
        assert rel_l2(got[:, c].cpu().numpy(), p.detach().cpu().numpy()) <= 1e-6, c
        s = opt.state[p]
        # the raw moments are stored every step with a regulariser: current without a sync
        assert rel_l2(st.m12[hidden][:, c].cpu().numpy(), s["exp_avg"].cpu().numpy()) <= 1e-6, c
        assert rel_l2(st.v12[hidden][:, c].cpu().numpy(), s["exp_avg_sq"].cpu().numpy()) <= 1e-6, c
    assert float((got[:, 3] - raw0[:, 3]).abs().min()) > 0.5 and float((got[:, 8:11] - raw0[:, 8:11]).abs().min()) > 0.05
    assert torch.equal(model.features[hidden], feat0)
    assert torch.equal(got[:, 0:3], raw0[:, 0:3]) and torch.equal(got[:, 4:8], raw0[:, 4:8])


# ---- 3. forms agree bit for bit -----------------------------------------------------------------------------------------------
def _pair(n=20000, seed=21, kw_a=None, kw_b=None):
    sc = scenes.scene_c1(n, seed)
    out = []
    for kw in (kw_a, kw_b):
        model = native.NativeGaussianModel(sc, device=DEV)
        out.append(native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, **kw))
    return out


def _views(W, H):
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1), (0.1, -1, 0), (0, 0.1, 1)]
    return [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=140.0) for k, d in enumerate(dirs)]


def _compare_forms(ref, other, names, synced_names=()):
    """Steps both trainers over five views from the same state (copied before every step) and compares `names` on the rows of
    waves that cannot receive a photometric gradient (bit for bit) and elsewhere (rtol 2e-5); `synced_names` the same after
    other.sync_moments().  The moments are copied with state_dict() / load_state_dict(), which marks a lazy trainer's waves current."""
    W, H = 160, 120
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    some_exact = 0
    for k, view in enumerate(_views(W, H)):
        other.load_state_dict(ref.state_dict())
        for name in ("raw", "features", "act"):
            _state(other)[name].copy_(_state(ref)[name])
        outs = [st.step(_batch(view, gt, host_pose=True))[1] for st in (ref, other)]
        for key in ("opacity_loss", "scale_loss"):
            assert torch.equal(outs[0][key], outs[1][key]), f"step {k}: {key}"
        exact = _gradient_free_waves(ref.raster, ref.model.num_gaussians)
        assert torch.equal(exact, _gradient_free_waves(other.raster, other.model.num_gaussians))
        some_exact += int(exact.sum())
        for name in names + synced_names:
            if name in synced_names:
                other.sync_moments()
            r, t = _state(ref)[name], _state(other)[name]
            assert torch.equal(r[exact], t[exact]), f"step {k}: {name} (rows that cannot receive a photometric gradient)"
            assert torch.allclose(r[~exact], t[~exact], rtol=2e-5, atol=1e-7), f"step {k}: {name} (rows in walked waves)"
    assert some_exact > 1000
    return some_exact


def test_regularised_two_pass_step_is_bit_identical_to_the_one_pass_step():
    reg = dict(lambda_opacity=0.01, lambda_scale=0.01)
    ref, ovl = _pair(kw_a=dict(overlap_optimizer=False, **reg), kw_b=dict(overlap_optimizer=True, **reg))
    ovl.raster.set_early_extra_percent(100)
    _compare_forms(ref, ovl, ("raw", "features", "m12", "v12", "m48", "v48", "act"))
    assert ovl.raster.stats()["side_stream_rows"] > 0


def test_regularised_lazy_moments_equal_eager_moments():
    reg = dict(lambda_opacity=0.01, lambda_scale=0.01, overlap_optimizer=True)
    eager, lazy = _pair(kw_a=dict(lazy_moments=False, **reg), kw_b=dict(lazy_moments=True, **reg))
    lazy.raster.set_early_extra_percent(100)
    eager.raster.set_early_extra_percent(100)
    assert lazy.lazy_moments and not eager.lazy_moments
    # the raw [N,12] moments are stored every step: bit-identical without a sync; the [N,48] ones are lazily decayed (one step
    # missed at most here, which the sync brings up to date bit for bit: beta^1 m = beta m + (1 - beta) 0)
    _compare_forms(eager, lazy, ("raw", "m12", "v12", "act"), synced_names=("m48", "v48"))


def test_switching_the_regulariser_mid_run_equals_eager_moments():
    """0 -> 0.01 -> 0 with lazy moments equals the same schedule with moments written every step (trainer syncs at each switch)."""
    base = dict(overlap_optimizer=True)
    eager, lazy = _pair(kw_a=dict(lazy_moments=False, **base), kw_b=dict(lazy_moments=True, **base))
    W, H = 160, 120
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    views = _views(W, H)
    lams = [0.0, 0.0, 0.01, 0.01, 0.01, 0.0, 0.0, 0.0]
    for k, lam in enumerate(lams):
        for st in (eager, lazy):
            st.lambda_opacity = st.lambda_scale = lam
            _, out = st.step(_batch(views[k % len(views)], gt, host_pose=True))
            assert ("opacity_loss" in out) == (lam != 0.0)
    lazy.sync_moments()
    for name in ("raw", "features", "m12", "v12", "m48", "v48"):
        assert rel_l2(_state(lazy)[name].cpu().numpy(), _state(eager)[name].cpu().numpy()) <= 2e-5, name


# ---- 4. exchange paths --------------------------------------------------------------------------------------------------------
def test_regularised_exchange_steps_equal_the_one_pass_step():
    sc = scenes.scene_c1(8000, 13)
    W, H = 128, 96
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(4)).to(DEV)
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1)]
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=110.0) for k, d in enumerate(dirs)]
    steppers = []
    for kw in (dict(), dict(fuse_epilogue=False, dp_exchange="sparse"), dict(fuse_epilogue=False, dp_exchange="dense")):
        model = native.NativeGaussianModel(sc, device=DEV)
        steppers.append(native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=False,
                                               lambda_opacity=0.01, lambda_scale=0.01, **kw))
    for view in views:
        outs = [st.step(_batch(view, gt))[1] for st in steppers]
        for o in outs[1:]:
            for key in ("opacity_loss", "scale_loss"):
                assert torch.equal(o[key], outs[0][key]), key
        assert not bool(steppers[1].g12.any())
    one = steppers[0]
    for st in steppers[1:]:
        for name in ("raw", "features", "m12", "v12"):
            assert rel_l2(_state(one)[name].cpu().numpy(), _state(st)[name].cpu().numpy()) <= 2e-5, name


# ---- 5. selective -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_regularised_selective_adam(fused):
    sc = scenes.scene_c1(3000, 23)
    W, H = 128, 96
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.1, 0.0, 0.0), (1.0, 0.2, 0.1)), fx=110.0)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    lam = 0.5
    mn = native.NativeGaussianModel(sc, device=DEV)
    tn = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0, selective=True, fused_sh_adam=fused,
                                lambda_opacity=lam, lambda_scale=lam)
    ma = model_mod.GaussianModel(sc, device=DEV)
    ta = train.TrainStep(ma, gut.Tracer({"render": {}}), scene_extent=1.0, optimizer_type="selective_adam", lambda_opacity=lam,
                         lambda_scale=lam)
    raw0 = mn.raw.clone()
    b = _batch(view, gt)
    la, oa = ta.step(b)
    ln, on = tn.step(b)
    assert abs(float(la) - float(ln)) <= 1e-5
    vis = on["mog_visibility"].reshape(-1) > 0
    assert 200 < int(vis.sum()) < 2800
    assert torch.equal(mn.raw[~vis], raw0[~vis])
    assert float(tn.m12[~vis].abs().max()) == 0.0
    raw_a = torch.cat([ma.positions, ma.density, ma.rotation, ma.scale], 1).detach()
    assert rel_l2(mn.raw[vis, :11].cpu().numpy(), raw_a[vis].cpu().numpy()) <= 2e-5
    assert float((mn.raw[vis, 3] - raw0[vis, 3]).abs().max()) > 0


# ---- 6. the recipe works ------------------------------------------------------------------------------------------------------
def _mcmc_run(lambda_opacity, steps=450):
    # (a Gaussian no view sees reaches opacity 0.005 from 0.5 after about 380 steps at N = 4000: Adam's second moment remembers the
    #  larger gradients of the first steps, so the logit moves by less than the learning rate per step later on)
    sc = scenes.scene_c1(4000, 12)
    outside = slice(0, 640)
    sc["positions"][outside] = sc["positions"][outside] * 0.5 + np.array([0.0, 0.0, -9.0])   # behind the camera
    sc["density"][outside] = 0.5
    W, H = 96, 72
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.0, 0.0, -4.0), (0, 0, 0)), fx=90.0)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    model = native.NativeGaussianModel(sc, device=DEV)
    loss_kw = dict(strategy.MCMC_LOSS, lambda_opacity=lambda_opacity)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True, **loss_kw)
    never = (10 ** 9, 10 ** 9 + 1, 1)
    mc = strategy.MCMCStrategy(st, max_n_gaussians=4000, schedule=dict(relocate=(50, 10 ** 6, 50), add=never, perturb=never))
    pos0 = model.raw[outside, 0:3].clone()
    dead = torch.zeros(640, dtype=torch.bool, device=DEV)
    for k in range(steps + 1):
        loss, out = st.step(_batch(view, gt, host_pose=True))
        dead |= torch.sigmoid(model.raw[outside, 3]) < 0.005
        mc.post_optimizer_step(k, 1.6e-4)
    st.sync_moments()
    assert all(bool(torch.isfinite(t).all()) for t in (model.raw, model.features, st.m12, st.v12, st.m48, st.v48))
    assert math.isfinite(float(loss))
    relocated = (model.raw[outside, 0:3] != pos0).any(1)
    return int(dead.sum()), int((relocated & dead).sum()), int(relocated.sum())


def test_mcmc_recipe_relocates_the_gaussians_no_view_sees():
    dead, dead_relocated, relocated = _mcmc_run(strategy.MCMC_LOSS["lambda_opacity"])
    assert dead >= 600 and dead_relocated == dead == relocated
    assert _mcmc_run(0.0) == (0, 0, 0)


# ---- 7. zero means unchanged --------------------------------------------------------------------------------------------------
def test_zero_coefficients_are_the_unregularised_step():
    plain, zero = _pair(kw_a=dict(overlap_optimizer=True), kw_b=dict(overlap_optimizer=True, lambda_opacity=0.0, lambda_scale=0.0))
    for st in (plain, zero):
        st.raster.set_early_extra_percent(100)
    W, H = 160, 120
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    for k, view in enumerate(_views(W, H)[:3]):
        for name, t in _state(zero).items():
            t.copy_(_state(plain)[name])
        outs = [st.step(_batch(view, gt, host_pose=True))[1] for st in (plain, zero)]
        assert "opacity_loss" not in outs[1] and "scale_loss" not in outs[1]
        exact = _gradient_free_waves(plain.raster, plain.model.num_gaussians)
        for name in ("raw", "features", "m12", "v12", "m48", "v48", "act"):
            r, t = _state(plain)[name], _state(zero)[name]
            assert torch.equal(r[exact], t[exact]), f"step {k}: {name}"
            assert torch.allclose(r[~exact], t[~exact], rtol=2e-5, atol=1e-7), f"step {k}: {name}"


# ---- 4b. two ranks on one card: the regulariser is counted once ---------------------------------------------------------------
DP_W, DP_H, DP_N = 80, 64, 600
DP_LAMBDA = dict(lambda_opacity=0.05, lambda_scale=1.0)


def _dp_views(world=2):
    eyes = ((0.3, -0.2, -3.5), (-2.2, 0.1, -2.6))
    return [make_view("pinhole", DP_W, DP_H, cams.look_at_c2w(eye, (0, 0, 0)), fx=80) for eye in eyes[:world]]


def _dp_gt(k):
    return torch.rand((1, DP_H, DP_W, 3), generator=torch.Generator().manual_seed(10 + k)).to(DEV)


def _dp_worker(rank, world, port, out_dir, form):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    sc = scenes.scene_c1(DP_N, 31)
    batch = to_batch(_dp_views(world)[rank], DEV); batch.rgb_gt = _dp_gt(rank)
    if form == "autograd":
        model = model_mod.GaussianModel(sc, device=DEV)
        stepper = train.TrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, world_size=world, **DP_LAMBDA)
    else:
        kw = dict(sparse=dict(dp_exchange="sparse"), dense=dict(dp_exchange="dense", dp_chunks=3, dp_chunk_min_rows=1),
                  unfused=dict(fused_sh_adam=False))[form]
        model = native.NativeGaussianModel(sc, device=DEV)
        stepper = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, world_size=world, rank=rank, **kw,
                                         **DP_LAMBDA)
    for _ in range(2):
        stepper.step(batch)
    if form == "autograd":
        raw = torch.cat([model.positions, model.density, model.rotation, model.scale], 1).detach().cpu()
    else:
        raw = model.raw[:, :11].cpu()
    torch.save(dict(raw=raw), os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier(); dist.destroy_process_group()


def _dp_reference(world, reg_count):
    """Single process, autograd: loss = mean over the views of the photometric loss + reg_count x the regulariser."""
    m = model_mod.GaussianModel(scenes.scene_c1(DP_N, 31), device=DEV)
    opt = torch.optim.Adam(m.param_groups(1.0), eps=1e-15)
    tracers = [gut.Tracer({"render": {}}) for _ in range(world)]
    for _ in range(2):
        loss = 0.0
        for k, view in enumerate(_dp_views(world)):
            out = tracers[k].render(m, to_batch(view, DEV), train=True)
            loss = loss + (1.0 / world) * losses.photometric_loss(out["pred_rgb"], _dp_gt(k))
        o, s = losses.regularisation_loss(m.get_density(), m.get_scale(), DP_LAMBDA["lambda_opacity"], DP_LAMBDA["lambda_scale"])
        loss = loss + reg_count * (o + s)
        loss.backward()
        opt.step(); opt.zero_grad(set_to_none=True)
    return torch.cat([m.positions, m.density, m.rotation, m.scale], 1).detach().cpu().numpy()


@pytest.mark.parametrize("form", ["sparse", "dense", "unfused", "autograd"])
def test_two_rank_regularised_step_counts_the_regulariser_once(tmp_path, form):
    """sparse: records + the unwalked-waves side stream; dense: the chunked dense exchange (600 rows -> 256 + 256 + 88, partials
    offset per chunk); unfused: gut_regularisation_gradient after the all-reduce's mean; autograd: TrainStep + all-reduce."""
    import socket
    import torch.multiprocessing as mp
    world = 2
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path), form), nprocs=world, join=True)
    r = [torch.load(f"{tmp_path}/r{k}.pt")["raw"] for k in range(world)]
    assert torch.equal(r[0], r[1])   # replicas stay identical
    once, twice = _dp_reference(world, 1.0), _dp_reference(world, float(world))
    got = r[0].numpy()
    # counting the regulariser `world` times would be seen: in the density logits, 10x the tolerance below
    assert rel_l2(twice[:, 3:4], once[:, 3:4]) > 1e-3
    for c in (slice(0, 3), slice(3, 4), slice(4, 8), slice(8, 11)):
        assert rel_l2(got[:, c], once[:, c]) <= 1e-4, (c, rel_l2(got[:, c], once[:, c]), rel_l2(twice[:, c], once[:, c]))
