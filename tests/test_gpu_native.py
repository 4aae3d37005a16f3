"""Native (fused) train step vs the torch-autograd train step: same scene, same view, one and three steps.
The two paths share the renderer; what differs is who does the activations, their backward and Adam.
Tolerances: parameters after a step agree to rel-L2 1e-5 (fp32, different exp/sigmoid implementations);
fused Adam alone matches torch.optim.Adam to 1e-6."""
import ctypes as C
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
model_mod = importlib.import_module("3dgrut_amd.model")
capi = importlib.import_module("3dgrut_amd._capi")
DEV = "cuda:0"


def test_fused_adam_matches_torch():
    """gut_adam_step, i.e. k_adam_step (the IEEE form: `/`, sqrtf), ONLY: five steps on benign values against torch.optim.Adam, block
    relative L2.  The trainer's fast-math forms (adam4, adam4_zero_grad, adam4_lazy) and every entry point's edges are held against
    float64 element by element in tests/test_gpu_step_elements.py."""
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn((1000, 12), generator=g)
    lr = np.linspace(1e-3, 5e-2, 12).astype(np.float32)
    cols = [torch.nn.Parameter(p0[:, i:i + 1].clone().cuda()) for i in range(12)]
    opt = torch.optim.Adam([dict(params=[c], lr=float(lr[i])) for i, c in enumerate(cols)], eps=1e-15)
    p = p0.clone().cuda(); m = torch.zeros_like(p); v = torch.zeros_like(p)
    lib = capi.load()
    st = torch.cuda.current_stream().cuda_stream
    for step in range(1, 6):
        grad = torch.randn((1000, 12), generator=g).cuda()
        for i, c in enumerate(cols):
            c.grad = grad[:, i:i + 1].clone()
        opt.step()
        rc = lib.gut_adam_step(C.c_void_p(st), 1000, 12, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                               (C.c_float * 12)(*lr.tolist()), 0.9, 0.999, 1e-15, step, None)
        assert rc == 0
    ref = torch.cat([c.detach() for c in cols], 1)
    assert rel_l2(p.cpu().numpy(), ref.cpu().numpy()) <= 1e-6


def test_selective_adam_semantics():
    """visibility==0 rows untouched; visible rows follow optimizers.cu:47-79 (no bias correction)."""
    g = torch.Generator().manual_seed(1)
    p = torch.randn((64, 4), generator=g).cuda(); p0 = p.clone()
    grad = torch.randn((64, 4), generator=g).cuda()
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    vis = (torch.arange(64) % 2 == 0).float().cuda()
    lib = capi.load()
    rc = lib.gut_adam_step(C.c_void_p(torch.cuda.current_stream().cuda_stream), 64, 4, p.data_ptr(), grad.data_ptr(), m.data_ptr(),
                           v.data_ptr(), (C.c_float * 4)(0.01, 0.01, 0.01, 0.01), 0.9, 0.999, 1e-8, 0, vis.data_ptr())
    assert rc == 0
    assert torch.equal(p[1::2], p0[1::2]) and float(m[1::2].abs().max()) == 0
    em = 0.1 * grad; ev = 0.001 * grad * grad
    exp = p0 - 0.01 * em / (ev.sqrt() + 1e-8)
    assert rel_l2(p[0::2].cpu().numpy(), exp[0::2].cpu().numpy()) <= 1e-6


@pytest.mark.parametrize("cols", [1, 3, 4, 45])
def test_selective_adam_class_follows_the_reference_kernel(cols):
    """3dgrut_amd.optimizers.SelectiveAdam (the reference's class surface, optimizers/__init__.py:46-131) on the parameter widths of
    the reference's model ([N,1] density, [N,3] positions / scale / albedo, [N,4] rotation, [N,45] specular): three steps against
    the formula of optimizers.cu:47-79 in torch — invisible rows keep parameters and moments bit for bit."""
    opt_mod = importlib.import_module("3dgrut_amd.optimizers")
    g = torch.Generator().manual_seed(cols)
    p0 = torch.randn((777, cols), generator=g)
    p = torch.nn.Parameter(p0.clone().to(DEV))
    opt = opt_mod.SelectiveAdam([dict(params=[p], lr=0.01, name="x")], eps=1e-15, betas=(0.9, 0.999))
    ref_p, ref_m, ref_v = p0.clone().double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double()
    for step in range(3):
        grad = torch.randn((777, cols), generator=g)
        vis = (torch.rand(777, generator=g) < 0.6)
        p.grad = grad.to(DEV)
        before = p.detach().clone()
        opt.step(vis.float().reshape(-1, 1).to(DEV))        # mog_visibility arrives as a float [N,1] tensor
        opt.zero_grad()
        gd = grad.double()
        b1, b2 = np.float32(0.9), np.float32(0.999)     # the kernel holds the betas in fp32: 1 - b2 = 0.0010000467
        m_new = float(b1) * ref_m + float(np.float32(1) - b1) * gd
        v_new = float(b2) * ref_v + float(np.float32(1) - b2) * gd * gd
        upd = -0.01 * m_new / (v_new.sqrt() + 1e-15)
        sel = vis[:, None].expand_as(ref_p)
        ref_p = torch.where(sel, ref_p + upd, ref_p); ref_m = torch.where(sel, m_new, ref_m); ref_v = torch.where(sel, v_new, ref_v)
        assert torch.equal(p.detach()[~vis.to(DEV)], before[~vis.to(DEV)])
    st = opt.state[p]
    assert rel_l2(p.detach().cpu().numpy(), ref_p.numpy()) <= 1e-6
    assert rel_l2(st["exp_avg"].cpu().numpy(), ref_m.numpy()) <= 1e-6 and rel_l2(st["exp_avg_sq"].cpu().numpy(), ref_v.numpy()) <= 1e-6
    with pytest.raises(RuntimeError, match="no CPU path"):
        q = torch.nn.Parameter(torch.zeros(4, 3)); q.grad = torch.ones(4, 3)
        opt_mod.SelectiveAdam([dict(params=[q], lr=0.01)]).step(torch.ones(4, 1))


@pytest.mark.parametrize("mode", ["dense", "compact", "one_pass"])
@pytest.mark.parametrize("steps", [1, 3])
def test_native_step_matches_autograd_step(steps, mode):
    """dense: K8 writes [N,12]+[N,48], two Adam launches; compact: K8c + fused SH-gradient/Adam kernel (the data-parallel
    layout); one_pass: epilogue + SH gradient + Adam in one kernel straight from the renderer's gradient rows."""
    fused = mode != "dense"
    sc = scenes.scene_c1(800, 21)
    view = make_view("pinhole", 96, 80, cams.look_at_c2w((0.2, -0.1, -3.5), (0, 0, 0)), fx=90)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, 80, 96, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    # autograd path
    ma = model_mod.GaussianModel(sc, device=DEV)
    ta = train.TrainStep(ma, gut.Tracer({"render": {}}), scene_extent=1.0)
    # native path
    mn = native.NativeGaussianModel(sc, device=DEV)
    tn = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0, fused_sh_adam=fused,
                                fuse_epilogue=(mode == "one_pass"))
    for _ in range(steps):
        la, _ = ta.step(batch)
        ln, _ = tn.step(batch)
        assert abs(float(la) - float(ln)) <= 1e-5
    raw = mn.raw.cpu().numpy()
    tol = 2e-5 if steps == 1 else 2e-4
    assert rel_l2(raw[:, 0:3], ma.positions.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 3:4], ma.density.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 4:8], ma.rotation.detach().cpu().numpy()) <= tol
    assert rel_l2(raw[:, 8:11], ma.scale.detach().cpu().numpy()) <= tol
    feats = torch.cat([ma.features_albedo, ma.features_specular], 1).detach().cpu().numpy()
    assert rel_l2(mn.features.cpu().numpy(), feats) <= tol


def test_cached_activation_is_dropped_when_raw_parameters_are_edited():
    """The fused Adam kernel leaves the next step's activated rows behind; an in-place edit of the raw parameters
    (densification, MCMC noise) must force a fresh activation, and a host-resident pose must give the same step."""
    sc = scenes.scene_c1(500, 4)
    view = make_view("pinhole", 64, 64, cams.look_at_c2w((0.0, 0.1, -3.5), (0, 0, 0)), fx=60)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, 64, 64, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    host_batch = to_batch(view, DEV)
    host_batch.rgb_gt = batch.rgb_gt
    host_batch.T_to_world = batch.T_to_world.cpu()
    runs = []
    for edit, b in ((False, batch), (True, batch), (True, host_batch)):
        mn = native.NativeGaussianModel(sc, device=DEV)
        tn = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0)
        tn.step(b)
        assert tn._act_key is not None
        if edit:
            mn.raw[:, 0:3].add_(0.05)      # in place: bumps the version counter
        act = tn.activate().clone()
        fresh = torch.empty_like(act)
        native._capi.load().gut_activate_pack(None, mn.num_gaussians, mn.raw.data_ptr(), fresh.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(act, fresh)
        loss, _ = tn.step(b)
        runs.append((float(loss), mn.raw.clone()))
    # device pose == host pose (parameters agree up to the summation order of the float atomics)
    assert runs[1][0] == runs[2][0] and torch.allclose(runs[1][1], runs[2][1], rtol=1e-4, atol=1e-6)
    assert runs[0][0] != runs[1][0]


def test_mcmc_relocation_kernel_matches_formula():
    """gut_mcmc_relocation vs the closed form of strategy/src/gaussian_mcmc.cu:33-73 evaluated in float64."""
    import math
    strategy = importlib.import_module("3dgrut_amd.strategy")
    mn = native.NativeGaussianModel(scenes.scene_c1(300, 2), device=DEV)
    mc = strategy.MCMCStrategy(native.NativeTrainStep(mn, gut.Tracer({"render": {}})), binom_n_max=51)
    g = torch.Generator().manual_seed(0)
    dens = (0.01 + 0.98 * torch.rand(300, generator=g)).cuda()
    scales = torch.rand((300, 3), generator=g).cuda() + 0.01
    ratios = torch.randint(1, 52, (300,), generator=g).int().cuda()
    nd, ns = mc._relocation(dens, scales, ratios)
    for i in range(0, 300, 7):
        n = int(ratios[i]); o = float(dens[i])
        no = 1 - (1 - o) ** (1.0 / n)
        den = sum(math.comb(a - 1, k) * ((-1) ** k / math.sqrt(k + 1)) * no ** (k + 1) for a in range(1, n + 1) for k in range(a))
        assert abs(float(nd[i]) - no) <= 2e-6
        assert abs(float(ns[i, 0]) - o / den * float(scales[i, 0])) <= 2e-4 * abs(o / den * float(scales[i, 0])) + 1e-6
    # end-to-end: relocation moves dead Gaussians onto live ones and zeroes their moments
    mn.raw[:40, 3] = -9.0
    assert mc.relocate(step=1) == 40 and float(torch.sigmoid(mn.raw[:, 3]).min()) > 0.004
    n0 = mn.num_gaussians
    assert mc.add_new(step=2) == int(1.05 * n0) - n0 and mn.num_gaussians == int(1.05 * n0)


def test_mcmc_relocation_kernel_on_what_the_reference_hands_it():
    """gut_mcmc_relocation on the tensors the reference's MCMCStrategy handed to ITS kernel in tests/golden/mcmc_golden.npz (three
    calls: a relocation and two additions; ratios up to the draws' multiplicity) against the recorded outputs — the kernel's
    closed form (gaussian_mcmc.cu:33-73) in float64, rounded to float32."""
    import os
    strategy = importlib.import_module("3dgrut_amd.strategy")
    S = np.load(os.path.join(os.path.dirname(__file__), "golden", "mcmc_golden.npz"))
    mn = native.NativeGaussianModel(scenes.scene_c1(64, 2), device=DEV)
    mc = strategy.MCMCStrategy(native.NativeTrainStep(mn, gut.Tracer({"render": {}})), binom_n_max=51)
    assert np.array_equal(mc.binoms.cpu().numpy(), S["binoms"])
    for i in range(int(S["kernel_calls"])):
        dens = torch.as_tensor(S[f"kernel{i}/opacities"]).reshape(-1).to(DEV)
        nd, ns = mc._relocation(dens, torch.as_tensor(S[f"kernel{i}/scales"]).to(DEV), torch.as_tensor(S[f"kernel{i}/ratios"]).to(DEV))
        np.testing.assert_allclose(nd.cpu().numpy(), S[f"kernel{i}/new_opacities"].reshape(-1), rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(ns.cpu().numpy(), S[f"kernel{i}/new_scales"], rtol=2e-4, atol=1e-9)
    assert max(int(S[f"kernel{i}/ratios"].max()) for i in range(3)) >= 3


def test_mcmc_perturb_kernel():
    """gut_mcmc_perturb against MCMCStrategy.perturb_gaussians restated with torch (mcmc.py:147-164, model.py:95-105, misc.py:69-90)
    for given standard-normal draws; its own draws (Philox4x32-10 keyed by seed and step, counter = row) are standard normal,
    reproducible, different from step to step, and the trainer's activated rows follow the positions."""
    strategy = importlib.import_module("3dgrut_amd.strategy")
    n = 200_000
    sc = scenes.scene_c1(n, 4)
    sc["density"] = np.random.default_rng(0).uniform(1e-4, 0.02, size=(n, 1)).astype(np.float32)   # around the gate's knee (0.005)
    mn = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0)
    st.activate()
    mc = strategy.MCMCStrategy(st, noise_lr=5e5, seed=3)
    raw0 = mn.raw.clone()
    unit = torch.randn((n, 3), generator=torch.Generator().manual_seed(1)).to(DEV)
    mc.unit_normal_fn = lambda shape, step: unit
    lr = 1.6e-4
    mc.perturb(lr, step=5)
    # the reference's lines, float64
    q = torch.nn.functional.normalize(raw0[:, 4:8].double(), dim=1)
    r, x, y, z = q.unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    S = torch.diag_embed(torch.exp(raw0[:, 8:11].double()))
    cov = R @ S @ S.transpose(1, 2) @ R.transpose(1, 2)
    dens = torch.sigmoid(raw0[:, 3:4].double())
    noise = unit.double() * (1 / (1 + torch.exp(-100 * ((1 - dens) - 0.995)))) * 5e5 * lr
    want = torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)
    got = (mn.raw[:, 0:3] - raw0[:, 0:3]).double()
    assert float(want.abs().max()) > 1e-4
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 2e-7        # (fp32 position ulp at |p| ~ 1: 6e-8)
    assert torch.equal(mn.raw[:, 3:], raw0[:, 3:])                                           # nothing but the positions moves
    assert torch.equal(st.act[:, 0:3], mn.raw[:, 0:3]) and torch.equal(st.activate()[:, 0:3], mn.raw[:, 0:3])
    # the kernel's own draws: identity rotations, unit scales, transparent Gaussians (gate ~ 1) -> displacement = draw * scale
    mn.raw.zero_(); mn.raw[:, 4] = 1.0; mn.raw[:, 3] = -30.0
    mc.unit_normal_fn = None
    draws = []
    for step in (7, 7, 8):
        mn.raw[:, 0:3] = 0.0
        mc.perturb(2e-6, step=step)                 # noise_lr * lr = 1
        draws.append(mn.raw[:, 0:3].clone())
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])
    gate = 1 / (1 + math.exp(-100 * ((1 - 1 / (1 + math.exp(30.0))) - 0.995)))
    u = draws[0].double() / gate
    assert abs(float(u.mean())) < 5e-3 and abs(float(u.var()) - 1.0) < 1e-2
    assert abs(float((u ** 4).mean()) - 3.0) < 0.1 and float(u.abs().max()) < 6.5                 # kurtosis of a normal; 600 k draws
    c = torch.corrcoef(torch.cat([u, draws[2].double() / gate], 1).T)
    assert float((c - torch.eye(6, dtype=c.dtype, device=c.device)).abs().max()) < 1e-2       # components and steps uncorrelated
    assert float((u[1:, 0] * u[:-1, 0]).mean().abs()) < 1e-2                                  # neighbouring rows too


def test_mcmc_strategy_on_the_live_trainer():
    """post_optimizer_step (mcmc.py:76-90) between native train steps, with the lazily decayed moments on: at an iteration the
    schedule selects for all three operations the dead Gaussians are relocated, 5 % are added (new rows: zero moments) and the
    near-transparent ones are perturbed; the trainer keeps stepping on the grown state and stays finite; at other iterations only
    the perturbation runs."""
    strategy = importlib.import_module("3dgrut_amd.strategy")
    sc = scenes.scene_c1(4000, 12)
    W, H = 96, 72
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.0, 0.0, 0.0), (1, 0, 0)), fx=90.0)
    b = to_batch(view, DEV); b.T_to_world = b.T_to_world.cpu()
    b.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True)
    mc = strategy.MCMCStrategy(st, max_n_gaussians=4300, schedule=dict(relocate=(2, 100, 3), add=(2, 100, 3), perturb=(0, 100, 1)))
    for _ in range(3):
        st.step(b)
    model.raw[100:160, 3] = -9.0                                  # sixty dead Gaussians
    pos0 = model.raw[:, 0:3].clone()
    assert mc.post_optimizer_step(3, 1.6e-4) == ["relocate", "add", "perturb"]
    assert model.num_gaussians == 4200 and st.m48.shape[0] == 4200 and float(torch.sigmoid(model.raw[:, 3]).min()) > 0.004
    assert not bool(st.m12[4000:].any()) and not bool(st.v48[4000:].any())
    assert bool((model.raw[:4000, 0:3] != pos0).any())
    for k in range(4, 9):
        loss, _ = st.step(b)
        done = mc.post_optimizer_step(k, 1.6e-4)
        assert done == (["relocate", "add", "perturb"] if k == 6 else ["perturb"])
    assert model.num_gaussians == 4300                              # the cap
    st.sync_moments()
    assert all(bool(torch.isfinite(t).all()) for t in (model.raw, model.features, st.m12, st.v12, st.m48, st.v48)) and math.isfinite(float(loss))


def test_colmap_scene_trains_end_to_end(tmp_path):
    """COLMAP sparse model -> per-view batches (pinhole + fisheye cameras) + initial Gaussians -> a few native train steps
    against images rendered from a perturbed copy: the loss must go down and every view must render."""
    import importlib
    import os
    io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
    from tests.test_cpu_io_strategy import _synthetic_colmap
    _synthetic_colmap(str(tmp_path), n_images=9, n_points=800)
    scene = io_colmap.ColmapScene(str(tmp_path), split="train", downsample_factor=4)
    init = scene.initial_gaussians(use_observation_points=True, observation_scale_factor=0.02, default_density=0.5)
    model = native.NativeGaussianModel(init, device=DEV)
    tracer = gut.Tracer({"render": {}})
    stepper = native.NativeTrainStep(model, tracer, scene_extent=scene.cameras_extent)
    # targets: the same Gaussians with different colours
    target = dict(init)
    target["features"] = init["features"].copy()
    target["features"][:, 0:3] = np.random.default_rng(1).uniform(-1, 1, size=(init["features"].shape[0], 3)).astype(np.float32)
    tm = native.NativeGaussianModel(target, device=DEV)
    batches = []
    for i in range(len(scene)):
        b = scene.batch(i, device=DEV)
        with torch.no_grad():
            out = tracer.render(tm, b, train=False)
        assert torch.isfinite(out["pred_rgb"]).all() and float(out["pred_opacity"].max()) > 0.0
        b.rgb_gt = out["pred_rgb"].detach().clone()
        batches.append(b)
    first = last = None
    for it in range(30):
        loss, _ = stepper.step(batches[it % len(batches)])
        if it < len(batches):
            first = float(loss) if first is None else first + float(loss)
        if it >= 30 - len(batches):
            last = float(loss) if last is None else last + float(loss)
    assert last < 0.8 * first, (first, last)


def _native_pair(n=20000, seed=21, **kw):
    sc = scenes.scene_c1(n, seed)
    steppers = []
    for overlap in (False, True):
        model = native.NativeGaussianModel(sc, device=DEV)
        tracer = gut.Tracer({"render": {"enable_kernel_timings": True}})
        steppers.append(native.NativeTrainStep(model, tracer, scene_extent=1.0, overlap_optimizer=overlap, **kw))
    return sc, steppers


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


def exact_wave_mask(cnt, unwalked):
    """Boolean [n]: rows of the waves the side stream owns with GUT_OPT_EARLY_EXTRA_PERCENT = 100: waves without any tile, and
    waves (with tiles) the forward walked nothing of."""
    n = cnt.numel()
    pad = (-n) % 64
    has = torch.nn.functional.pad(cnt != 0, (0, pad)).view(-1, 64).any(1)
    unw = torch.nn.functional.pad(unwalked, (0, pad), value=True).view(-1, 64).all(1)
    return ((~has) | unw).repeat_interleave(64)[:n]


def test_early_optimiser_pass_is_bit_identical_to_the_one_pass_kernel():
    """gut_optimize_rows_without_gradient (rows without tiles, side stream, under the compositing kernels) followed by
    gut_optimize_after_bwd (rows with tiles) leaves EXACTLY the parameters, moments and activations of the one-pass kernel,
    over several steps with changing views (so rows change sides between steps)."""
    sc, (ref, ovl) = _native_pair()
    W, H = 160, 120
    g = torch.Generator().manual_seed(5)
    gt = torch.rand((1, H, W, 3), generator=g).to(DEV)
    # cameras INSIDE the cloud looking in different directions: every view sees a different subset of the Gaussians
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1), (0.1, -1, 0), (0, 0.1, 1)]
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=140.0) for k, d in enumerate(dirs)]
    some_without_tiles = some_unwalked_with_tiles = 0
    ovl.raster.set_early_extra_percent(100)
    state = lambda st: dict(raw=st.model.raw, features=st.model.features, m12=st.m12, v12=st.v12, m48=st.m48, v48=st.v48, act=st.act)
    for k, view in enumerate(views):
        # both start every step from the same bits (the rows WITH tiles pick up run-to-run differences in the last bits from
        # the float atomics of the compositing backward, whichever optimiser form follows)
        for name, t in state(ovl).items():
            t.copy_(state(ref)[name])
        for st in (ref, ovl):
            b = to_batch(view, DEV)
            b.T_to_world = b.T_to_world.cpu()
            b.rgb_gt = gt
            st.step(b)
        cnt = ovl.raster.debug_buffer("tiles_count")
        assert torch.equal(cnt, ref.raster.debug_buffer("tiles_count"))
        early = cnt == 0
        some_without_tiles += int(early.sum())
        # rows of 64-row waves in which the forward walked no Gaussian cannot receive a gradient either (the backward is bounded
        # by the forward's per-tile depth): the side stream's second launch takes those waves too, and they must come out
        # bit-identical as well
        unwalked = _rows_in_unwalked_waves(ovl.raster, cnt.numel())
        assert torch.equal(unwalked, _rows_in_unwalked_waves(ref.raster, cnt.numel()))
        some_unwalked_with_tiles += int((unwalked & ~early).sum())
        exact = early | unwalked
        for name, t in state(ovl).items():
            r = state(ref)[name]
            assert torch.equal(r[exact], t[exact]), f"step {k}: {name} (rows that cannot receive a gradient)"
            assert torch.allclose(r[~exact], t[~exact], rtol=2e-5, atol=1e-7), f"step {k}: {name} (rows in walked waves)"
        st_ = ovl.raster.stats()
        assert st_["side_stream_rows"] == int(exact_wave_mask(cnt, unwalked).sum()) and ref.raster.stats()["side_stream_rows"] == 0
        # rows that had a gradient earlier and have no tiles now keep moving on their momentum (dense Adam semantics)
        if k > 0:
            coasting = early & ever_tiles
            assert int(coasting.sum()) > 0
            assert float((state(ovl)["raw"][coasting] - before[coasting]).abs().max()) > 0
            # rows that never had a gradient are a fixed point of the zero-gradient update
            dormant = early & ~ever_tiles
            if k < 3:
                assert int(dormant.sum()) > 0
            assert torch.equal(state(ovl)["raw"][dormant], before[dormant])
            assert not state(ovl)["m48"][dormant].any() and not state(ovl)["v12"][dormant].any()
        ever_tiles = (~early) if k == 0 else (ever_tiles | ~early)
        before = state(ovl)["raw"].clone()
    assert some_without_tiles > 1000 and some_unwalked_with_tiles > 1000
    kt = ovl.raster.kernel_times()
    assert kt["optimizer_early"] > 0 and kt["optimizer"] > 0 and ref.raster.kernel_times()["optimizer_early"] < 0


def test_sparse_gradient_records_equal_the_dense_epilogue():
    """gut_compact_gradient_rows -> gut_scatter_gradient_records rebuilds exactly the [N,12] raw-parameter gradient and the
    masked dL/dRGB that the dense compact epilogue (GUT_BWD_COMPACT_RADIANCE_GRADS) writes; ids are unique, rows without a
    gradient get no record, and the handle's gradient rows are left consumed."""
    sc = scenes.scene_c1(5000, 9)
    W, H = 96, 80
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.2, 0.1, -3.0), (0, 0, 0)), fx=90.0)
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fuse_epilogue=False)
    b = to_batch(view, DEV)
    rgba, dist_, hits, vis = st.forward(b)
    g = torch.Generator().manual_seed(3)
    rgba_grad = torch.randn(rgba.shape, generator=g).to(DEV)
    _, sensor, poses, _, _ = st._ctx
    m = st.model
    args = (st.step_id, m.n_active_features, st.act, m.features, b.rays_ori.contiguous(), b.rays_dir.contiguous(), None, sensor,
            poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1], rgba, rgba_grad,
            dist_, None)
    n = m.num_gaussians
    g12 = torch.empty((n, 12), device=DEV); mrgb = torch.empty((n, 3), device=DEV)
    st.raster.trace_bwd(*args, raw_parameter_grads=True, compact_radiance_grads=True, out=(g12, mrgb))
    st.raster.trace_bwd(*args, skip_epilogue=True)
    rec = torch.full((n, 16), float("nan"), device=DEV); cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    st.raster.compact_gradient_rows(st.act, rec, cnt)
    c = int(cnt.item())
    ids = rec[:c, 11].contiguous().view(torch.int32).long()
    assert 0 < c < n and ids.unique().numel() == c and int(ids.max()) < n
    has_grad = (g12.abs().sum(1) + mrgb.abs().sum(1)) > 0
    assert set(ids.tolist()) >= set(torch.nonzero(has_grad).reshape(-1).tolist())   # (a record may carry an all-zero chained row)
    # the consumed rows are zero again: a second backward + compaction finds the same gradients, not twice their sum
    st.raster.trace_bwd(*args, skip_epilogue=True)
    rec2 = torch.empty((n, 16), device=DEV); cnt2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    st.raster.compact_gradient_rows(st.act, rec2, cnt2)
    assert int(cnt2.item()) == c
    o1, o2 = torch.argsort(ids), torch.argsort(rec2[:c, 11].contiguous().view(torch.int32).long())
    close = lambda a, b: rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5   # two backward runs differ by float-atomic noise
    assert close(rec[:c][o1][:, :11], rec2[:c][o2][:, :11]) and close(rec[:c][o1][:, 12:], rec2[:c][o2][:, 12:])
    acc = torch.zeros((n, 12), device=DEV); slab = torch.zeros((n, 3), device=DEV)
    lib = st._lib
    s_ = torch.cuda.current_stream().cuda_stream
    assert lib.gut_scatter_gradient_records(C.c_void_p(s_), rec.data_ptr(), c, n, acc.data_ptr(), slab.data_ptr()) == 0
    assert close(acc, g12) and close(slab, mrgb)   # the chain arithmetic is the same
    assert bool((rec[:c, 15] == 0).all())
    # a second scatter of the same view accumulates (that is how several views sum up) ...
    assert lib.gut_scatter_gradient_records(C.c_void_p(s_), rec.data_ptr(), c, n, acc.data_ptr(), slab.data_ptr()) == 0
    assert close(acc, 2 * g12) and close(slab, mrgb)
    # ... and a record whose id is not a row of the model is dropped, not stored through
    bad = rec[:1].clone(); bad[0, 11] = torch.tensor([n + 5], dtype=torch.int32).view(torch.float32)[0]
    before = acc.clone()
    assert lib.gut_scatter_gradient_records(C.c_void_p(s_), bad.data_ptr(), 1, n, acc.data_ptr(), slab.data_ptr()) == 0
    assert torch.equal(acc, before)
    with pytest.raises(RuntimeError, match="no backward context"):
        st.raster.compact_gradient_rows(st.act, rec, cnt)


def test_sparse_exchange_step_equals_the_one_pass_step():
    """dp_exchange="sparse" with one rank (records -> scatter -> k_sh_adam<false> with self-clearing accumulators) leaves the
    parameters of the fused one-pass step over several views, and the dense accumulators all-zero after every step."""
    sc = scenes.scene_c1(8000, 13)
    W, H = 128, 96
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(4)).to(DEV)
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1)]
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=110.0) for k, d in enumerate(dirs)]
    steppers = []
    for kw in (dict(), dict(fuse_epilogue=False, dp_exchange="sparse"), dict(fuse_epilogue=False, dp_exchange="dense")):
        model = native.NativeGaussianModel(sc, device=DEV)
        steppers.append(native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=False, **kw))
    hooked = []
    steppers[1].post_backward_hook = lambda pg, cam: hooked.append(pg.clone())
    dense_hook = []
    steppers[2].post_backward_hook = lambda pg, cam: dense_hook.append(pg.clone())
    for view in views:
        for st in steppers:
            b = to_batch(view, DEV); b.rgb_gt = gt
            st.step(b)
        sp = steppers[1]
        assert not bool(sp.g12.any()) and not bool(sp.mrgb[0].any()) and 0 < sp.exchanged_records < 8000
        assert rel_l2(hooked[-1].cpu().numpy(), dense_hook[-1].cpu().numpy()) <= 1e-5
    one, sp, de = steppers
    for a, b_ in ((one.model.raw, sp.model.raw), (one.model.features, sp.model.features), (one.m48, sp.m48), (one.v12, sp.v12),
                  (de.model.raw, sp.model.raw), (de.model.features, sp.model.features)):
        assert rel_l2(a.cpu().numpy(), b_.cpu().numpy()) <= 2e-5


def test_walked_wave_flags_match_the_walked_list_prefixes():
    """gut_mark_walked_waves: flag[w] == 1 exactly for the 64-row waves that hold a Gaussian among the first
    tile_traversed_fwd[tile] entries of some tile's ordered list — and every Gaussian the backward gives a gradient to lies in
    such a wave (the backward compositor is bounded by the forward's depth)."""
    sc = scenes.scene_c1(20000, 23)
    W, H = 160, 120
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.05, 0.0, 0.02), (1, 0, 0)), fx=140.0)   # camera inside the cloud
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fuse_epilogue=False)
    b = to_batch(view, DEV)
    rgba, dist_, hits, vis = st.forward(b)
    n = model.num_gaussians
    flags = torch.full(((n + 63) // 64,), 7, dtype=torch.uint8, device=DEV)
    s_ = torch.cuda.current_stream().cuda_stream
    assert st._lib.gut_mark_walked_waves(st.raster._handle, C.c_void_p(s_), flags.data_ptr()) == 0
    unwalked_rows = _rows_in_unwalked_waves(st.raster, n)
    expect = ~torch.nn.functional.pad(unwalked_rows, (0, (-n) % 64), value=True).view(-1, 64).all(1)
    assert torch.equal(flags.bool(), expect) and int(flags.max()) == 1
    assert 0 < int(expect.sum()) < expect.numel()
    # gradients only inside flagged waves
    _, sensor, poses, _, _ = st._ctx
    m = st.model
    rgba_grad = torch.randn(rgba.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    args = (st.step_id, m.n_active_features, st.act, m.features, b.rays_ori.contiguous(), b.rays_dir.contiguous(), None, sensor,
            poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1], rgba, rgba_grad,
            dist_, None)
    g12 = torch.empty((n, 12), device=DEV); mrgb = torch.empty((n, 3), device=DEV)
    st.raster.trace_bwd(*args, raw_parameter_grads=True, compact_radiance_grads=True, out=(g12, mrgb))
    has_grad = (g12.abs().sum(1) + mrgb.abs().sum(1)) > 0
    assert int(has_grad.sum()) > 0 and not bool((has_grad & unwalked_rows).any())


def test_placement_tuning_moves_the_state_without_changing_it():
    """NativeTrainStep.tune_placement: the no-op pass of the side-stream kernel (zero learning rates, beta = 1) and the moves to
    fresh memory leave parameters, moments and activations bit-identical, and the stepper keeps training on them."""
    sc = scenes.scene_c1(30000, 5)
    W, H = 96, 80
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.2, 0.1, -3.0), (0, 0, 0)), fx=90.0)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    steppers = []
    for _ in range(2):
        model = native.NativeGaussianModel(sc, device=DEV)
        steppers.append(native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=False))
    ref, tuned = steppers
    for st in steppers:
        b = to_batch(view, DEV); b.rgb_gt = gt
        st.step(b)                       # non-trivial moments
    state = lambda st: dict(raw=st.model.raw, features=st.model.features, m12=st.m12, v12=st.v12, m48=st.m48, v48=st.v48)
    before = {k: v.clone() for k, v in state(tuned).items()}
    ptrs = {k: v.data_ptr() for k, v in state(tuned).items()}
    act_before = tuned.activate().clone()
    times = tuned.tune_placement(attempts=2)
    # the start + at most 2 per big tensor; the first trial that is > 5 % faster ends the search
    assert 2 <= len(times) <= 7 and all(t > 0 for t in times) and tuned.placement_trials_ms == times
    assert all(t >= 0.95 * times[0] for t in times[1:-1])
    for k, v in state(tuned).items():
        assert torch.equal(v, before[k]), k
    moved = [k for k in ptrs if state(tuned)[k].data_ptr() != ptrs[k]]
    assert set(moved) <= {"features", "m48", "v48"} and len(moved) <= 1   # only one of the three [N,48] tensors is ever re-placed ...
    assert bool(moved) == (min(times[1:]) < 0.95 * times[0])            # ... and only for a pass that got > 5 % faster
    assert torch.equal(tuned.activate(), act_before)
    for st in steppers:
        b = to_batch(view, DEV); b.rgb_gt = gt
        st.step(b)
    for k in before:   # (two separate runs of the backward: equal up to its float-atomic noise)
        assert rel_l2(state(tuned)[k].cpu().numpy(), state(ref)[k].cpu().numpy()) <= 1e-4, k


def test_half_applied_optimiser_step_is_an_error():
    sc, (_, ovl) = _native_pair(n=500)
    view = make_view("pinhole", 64, 48, cams.look_at_c2w((0, 0, -4), (0, 0, 0)), fx=64.0)
    b = to_batch(view, DEV)
    ovl.forward(b)
    m = ovl.model
    args = (m.raw, ovl.m12, ovl.v12, m.features, ovl.m48, ovl.v48, ovl.lr12, ovl.lr48, ovl.betas, ovl.eps, 1, ovl.act)
    ovl.raster.optimize_rows_without_gradient(*args)
    with pytest.raises(RuntimeError, match="already called"):
        ovl.raster.optimize_rows_without_gradient(*args)
    with pytest.raises(RuntimeError, match="half applied"):
        ovl.forward(b)


def test_a_failing_step_is_finished_with_a_zero_gradient():
    """Something raises between the side-stream optimiser pass and gut_optimize_after_bwd (here: a loss that rejects its
    target): NativeTrainStep.step finishes the iteration for every other row with a zero gradient
    (gut_optimize_finish_without_gradient), the error still reaches the caller, the handle renders again, and the state is
    EXACTLY one zero-gradient Adam step of every row — what gut_adam_unwalked_waves computes with all-zero wave flags."""
    sc, (_, ovl) = _native_pair(n=3000)
    view = make_view("pinhole", 96, 64, cams.look_at_c2w((0.1, 0, -3.5), (0, 0, 0)), fx=90.0)
    good = to_batch(view, DEV); good.rgb_gt = torch.rand((1, 64, 96, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    ovl.step(good); ovl.step(good)                       # non-trivial moments
    ovl.sync_moments()                                   # (lazily decayed moments: bring the stored ones up to date before cloning them)
    n = ovl.model.num_gaussians
    state = lambda st: dict(raw=st.model.raw, features=st.model.features, m12=st.m12, v12=st.v12, m48=st.m48, v48=st.v48)
    exp = {k: v.clone() for k, v in state(ovl).items()}
    exp_act = torch.empty_like(ovl.act)
    lib = capi.load()
    f32p = C.POINTER(C.c_float)
    rc = lib.gut_adam_unwalked_waves(C.c_void_p(torch.cuda.current_stream().cuda_stream), n, torch.zeros((n + 63) // 64, dtype=torch.uint8, device=DEV).data_ptr(),
                                     exp["raw"].data_ptr(), exp["m12"].data_ptr(), exp["v12"].data_ptr(), exp["features"].data_ptr(),
                                     exp["m48"].data_ptr(), exp["v48"].data_ptr(), ovl.lr12.ctypes.data_as(f32p), ovl.lr48.ctypes.data_as(f32p),
                                     ovl.betas[0], ovl.betas[1], ovl.eps, ovl.step_id + 1, exp_act.data_ptr())
    assert rc == 0
    bad = to_batch(view, DEV); bad.rgb_gt = "not a tensor"
    with pytest.raises(AttributeError):
        ovl.step(bad)
    assert ovl.step_id == 3                              # the iteration WAS applied (with a zero gradient), although step() raised
    ovl.sync_moments()
    torch.cuda.synchronize()
    for k, v in state(ovl).items():
        assert torch.equal(v, exp[k]), k
    ovl.forward(good)                                    # the handle is usable again ...
    assert torch.equal(ovl.act, exp_act)                 # ... and the activation rows follow the updated parameters
    ovl.step(good)
    assert bool(torch.isfinite(ovl.model.raw).all())
    # a plain (non-SKIP_EPILOGUE) backward after the side-stream call is rejected at once, not at the next forward
    ovl.forward(good)
    m = ovl.model
    ovl.raster.optimize_rows_without_gradient(m.raw, ovl.m12, ovl.v12, m.features, ovl.m48, ovl.v48, ovl.lr12, ovl.lr48, ovl.betas, ovl.eps,
                                              ovl.step_id + 1, ovl.act)
    b_, sensor, poses, rgba, dist_ = ovl._ctx
    with pytest.raises(RuntimeError, match="GUT_BWD_SKIP_EPILOGUE"):
        ovl.raster.trace_bwd(ovl.step_id, m.n_active_features, ovl.act, m.features, b_.rays_ori.contiguous(), b_.rays_dir.contiguous(), None,
                             sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1],
                             rgba, torch.zeros_like(rgba), dist_, None)
    ovl.raster.finish_optimizer_step_without_gradient()
    ovl.forward(good)


def test_lazy_moment_decay_equals_writing_the_moments_every_step():
    """GutLazyMoments: waves that cannot receive a gradient read their moments, bring them up to date in registers and do not write
    them back; the next reader multiplies by beta^(steps missed).  Against the same trainer writing both moments every step
    (lazy_moments=False = torch.optim.Adam's schedule of roundings), over eight steps on changing views, from non-zero moments on
    every row: rows no view ever touched — no float-atomic noise, so a clean comparison — agree to the rounding of beta^k against k
    successive multiplications; the stored moments really are stale in between and current after sync_moments()."""
    sc = scenes.scene_c1(20000, 23)
    W, H = 160, 120
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1), (1, 0.1, 0), (0.1, -1, 0), (0, 0.1, 1), (1, 0, 0.1), (-1, 0.2, 0)]
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=140.0) for k, d in enumerate(dirs)]
    steppers = {}
    for lazy in (False, True):
        model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True, lazy_moments=lazy)
        g = torch.Generator(device=DEV).manual_seed(7)
        for m_, v_ in ((st.m12, st.v12), (st.m48, st.v48)):
            m_.normal_(0.0, 1e-4, generator=g)
            v_.fill_(1e-6)
        steppers[lazy] = st
    eager, lazy = steppers[False], steppers[True]
    assert lazy.lazy_moments and not eager.lazy_moments and eager.wave_step is None
    m48_0 = lazy.m48.clone()
    touched = torch.zeros(20000, dtype=torch.bool, device=DEV)
    stale_seen = 0
    for k, view in enumerate(views):
        for st in (eager, lazy):
            b = to_batch(view, DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
            st.step(b)
        cnt = lazy.raster.debug_buffer("tiles_count")
        assert torch.equal(cnt, eager.raster.debug_buffer("tiles_count"))
        owned = exact_wave_mask(cnt, _rows_in_unwalked_waves(lazy.raster, 20000))
        touched |= ~owned
        # a wave that has not been able to receive a gradient so far still holds its INITIAL moments, k + 1 steps stale
        never = ~touched
        assert torch.equal(lazy.m48[never], m48_0[never])
        stale_seen = max(stale_seen, int(lazy.step_id - lazy.wave_step.min()))
    assert stale_seen == len(views) and int(never.sum()) > 2000
    lazy.sync_moments()
    assert int(lazy.wave_step.min()) == lazy.step_id == len(views)
    for name in ("m12", "v12", "m48", "v48"):
        a, b = getattr(eager, name)[never], getattr(lazy, name)[never]
        assert torch.allclose(a, b, rtol=2e-6, atol=0.0), name              # beta^8 in one rounding vs eight
        assert not torch.equal(b, dict(m48=m48_0[never]).get(name, b + 1))    # ... and they did decay
    for name, t in (("raw", lazy.model.raw), ("features", lazy.model.features), ("act", lazy.act)):
        r = dict(raw=eager.model.raw, features=eager.model.features, act=eager.act)[name]
        assert torch.allclose(r[never], t[never], rtol=1e-6, atol=1e-7), name
        assert float((r[~never] - t[~never]).abs().max()) < 0.2              # (rows with gradients: float-atomic noise through Adam)
    # sync is idempotent and invisible to the next step: two more steps, one of them right after a sync
    snap = {k: getattr(lazy, k).clone() for k in ("m12", "v12", "m48", "v48")}
    lazy.sync_moments()
    assert all(torch.equal(getattr(lazy, k), v) for k, v in snap.items())


def test_lazy_moments_over_more_steps_than_the_decay_tables_hold():
    """1100 train steps on rotating views (the beta^k tables hold 1024 entries; the trainer brings every wave up to date every 512
    steps): no wave's missed steps ever run off the tables, everything stays finite, and the rows no view ever touched agree with
    the trainer that writes its moments every step — second moments to 1e-5 (beta2^1100 = 0.33 in three table look-ups against 1100
    roundings), parameters to 1e-6."""
    sc = scenes.scene_c1(20000, 31)
    W, H = 96, 72
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    dirs = [(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1), (0.1, -1, 0)]
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=90.0) for k, d in enumerate(dirs)]
    batches = []
    for v in views:
        b = to_batch(v, DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
        batches.append(b)
    steppers = {}
    for lazy in (False, True):
        model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True, lazy_moments=lazy)
        g = torch.Generator(device=DEV).manual_seed(7)
        for m_, v_ in ((st.m12, st.v12), (st.m48, st.v48)):
            m_.normal_(0.0, 1e-4, generator=g)
            v_.fill_(1e-6)
        steppers[lazy] = st
    eager, lazy = steppers[False], steppers[True]
    touched = torch.zeros(20000, dtype=torch.bool, device=DEV)
    worst_missed = 0
    for k in range(1100):
        for st in (eager, lazy):
            st.step(batches[k % 4])
        if k < 4:
            cnt = lazy.raster.debug_buffer("tiles_count")
            touched |= ~exact_wave_mask(cnt, _rows_in_unwalked_waves(lazy.raster, 20000))
        if k % 100 == 99 or k in (510, 511, 512, 1023, 1024):
            worst_missed = max(worst_missed, int(lazy.step_id - lazy.wave_step.min()))
    assert lazy.step_id == 1100 and worst_missed <= 512 < lazy.LAZY_TABLE        # synced at 512 and 1024
    lazy.sync_moments()
    never = ~touched
    assert int(never.sum()) > 2000
    for st in (eager, lazy):
        assert all(bool(torch.isfinite(t).all()) for t in (st.model.raw, st.model.features, st.m12, st.v12, st.m48, st.v48, st.act))
    for name in ("v12", "v48"):
        assert torch.allclose(getattr(eager, name)[never], getattr(lazy, name)[never], rtol=1e-5, atol=0.0), name
    assert torch.allclose(eager.model.raw[never], lazy.model.raw[never], rtol=1e-6, atol=1e-7)
    assert torch.allclose(eager.model.features[never], lazy.model.features[never], rtol=1e-6, atol=1e-7)


def test_checkpoint_resume_beyond_the_decay_tables():
    """the public moment tensors are stale under the lazy decay and `wave_step` belongs to the step counter.
    state_dict() syncs before it exports; load_state_dict() / set_step() re-base every wave; a trainer resumed at step 1500 (beyond
    the 1024-entry beta^k tables) continues exactly like the one that never stopped and like the trainer that writes its moments
    every step; a resume that bypasses them (moments copied, wave_step left behind) is REPORTED instead of silently multiplying
    every moment by beta^1023."""
    sc = scenes.scene_c1(20000, 33)
    W, H = 96, 72
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(9)).to(DEV)
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.05 * k, 0.0, 0.02 * k), d), fx=90.0)
             for k, d in enumerate([(1, 0, 0), (-1, 0.2, 0), (0, 1, 0.1)])]
    batches = []
    for v in views:
        b = to_batch(v, DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
        batches.append(b)

    def make(lazy):
        model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True, lazy_moments=lazy)
        g = torch.Generator(device=DEV).manual_seed(7)
        for m_, v_ in ((st.m12, st.v12), (st.m48, st.v48)):
            m_.normal_(0.0, 1e-4, generator=g)
            v_.fill_(1e-6)
        return st

    eager, lazy = make(False), make(True)
    for st in (eager, lazy):
        st.set_step(1500)                       # a run that is 1500 steps old (the moments keep their values)
        assert st.step_id == 1500 and (st.wave_step is None or int(st.wave_step.min()) == 1500)
    for k in range(6):
        for st in (eager, lazy):
            st.step(batches[k % 3])
    assert int(lazy.wave_step.min()) < lazy.step_id            # some waves ARE behind: the stored moments are stale ...
    stale = lazy.m48.clone()
    sd = lazy.state_dict()                                     # ... and the checkpoint holds current ones
    assert sd["step"] == 1506 and not torch.equal(stale, sd["exp_avg_features"])
    assert torch.allclose(sd["exp_avg_sq_features"], eager.v48, rtol=2e-6, atol=0.0)
    _d = (sd["exp_avg_features"] - eager.m48).abs()
    # Two GPU runs, not a run against a reference: the backward accumulates each Gaussian's gradient with float atomics in an order
    # that differs from run to run, so an element of the first moment carries an ABSOLUTE noise of about 0.1 x 2^-24 x sum |terms| per
    # step (a few 1e-10 for this scene's colour gradients) whatever its own size, and an element that happens to sit near zero cannot
    # meet a purely relative bound (one such element in 960 k failed atol 1e-12 once in eight runs of the suite).  2e-9 is 2e-5 of the
    # moments' typical magnitude (1e-4).
    assert torch.allclose(sd["exp_avg_features"], eager.m48, rtol=1e-5, atol=2e-9), \
        f"max abs diff {float(_d.max()):.3e} at |value| {float(eager.m48.flatten()[_d.argmax()].abs()):.3e}, {int((_d > 1e-5 * eager.m48.abs() + 1e-12).sum())} elements over"
    # resume into a fresh trainer
    resumed = make(True)
    resumed.model.raw.copy_(lazy.model.raw); resumed.model.features.copy_(lazy.model.features)
    resumed.load_state_dict(sd)
    assert resumed.step_id == 1506 and int(resumed.wave_step.min()) == 1506
    for k in range(6, 12):
        for st in (eager, lazy, resumed):
            st.step(batches[k % 3])
    for st in (lazy, resumed):
        st.sync_moments()
    # the resumed run IS the uninterrupted one, up to the float-atomic order of the two trainers' backward passes
    for name in ("m12", "v12", "m48", "v48"):
        assert torch.allclose(getattr(lazy, name), getattr(resumed, name), rtol=2e-5, atol=1e-10), name
    assert torch.allclose(lazy.model.raw, resumed.model.raw, rtol=1e-6, atol=1e-7)
    assert torch.allclose(lazy.model.features, resumed.model.features, rtol=1e-6, atol=1e-7)
    assert torch.allclose(eager.model.features, lazy.model.features, rtol=1e-5, atol=1e-7)
    assert torch.allclose(eager.v48, lazy.v48, rtol=1e-5, atol=0.0)
    # the unsafe resume: moments copied into a fresh trainer, the private counter forced, wave_step left at 0
    bad = make(True)
    bad.model.raw.copy_(lazy.model.raw); bad.model.features.copy_(lazy.model.features)
    bad._step_id = 1512
    bad.step(batches[0])
    with pytest.raises(RuntimeError, match="missed 1024 or more steps"):
        bad.sync_moments()


def test_dense_chunk_exchange_reports_a_decay_table_overrun():
    """The dense-exchange chunk loop hands every chunk the trainer's overrun word (GutLazyMoments.d_overrun), like every other
    optimiser path: three chunks (0,1024), (1024,2048), (2048,3000) — the last ends in a partial wave; collectives skipped without a
    process group.  Two ordinary steps leave nothing to report; a step counter forced 1500 steps ahead of wave_step (the unsafe resume
    of test_checkpoint_resume_beyond_the_decay_tables) is REPORTED by sync_moments() — the kernel clamps the table index, so this is
    a reported condition, not a fault."""
    sc = scenes.scene_c1(3000, 35)
    W, H = 128, 96
    b = to_batch(make_view("pinhole", W, H, cams.look_at_c2w((0.3, 0.1, -3.5), (0, 0, 0)), fx=120.0), DEV)
    b.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(10)).to(DEV)
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fuse_epilogue=False, dp_exchange="dense",
                                dp_chunks=3, dp_chunk_min_rows=1, lazy_moments=True)
    st.force_exchange = True
    st.resize_workspace()
    assert st.chunks == [(0, 1024), (1024, 2048), (2048, 3000)] and st.lazy_moments
    for _ in range(2):
        st.step(b)
    st.sync_moments()                      # healthy: nothing ran off the tables
    assert int(st.wave_step.max()) <= 2
    st._step_id = 1512                     # wave_step stays behind
    st.step(b)
    with pytest.raises(RuntimeError, match="missed 1024 or more steps"):
        st.sync_moments()


def test_spatial_storage_order_is_transparent():
    """NativeGaussianModel(spatial_order=True) only permutes the rows: same image, and after two train steps the parameters
    are those of the scene-order model, row for row through `permutation` (up to the float-atomic noise of the backward);
    restore_spatial_order() after an in-place change keeps the optimiser state attached to its rows."""
    sc = scenes.scene_c1(6000, 17)
    W, H = 128, 96
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.3, 0.1, -3.5), (0, 0, 0)), fx=120.0)
    g = torch.Generator().manual_seed(2)
    gt = torch.rand((1, H, W, 3), generator=g).to(DEV)
    steppers = []
    for spatial in (False, True):
        model = native.NativeGaussianModel(sc, device=DEV, spatial_order=spatial)
        steppers.append(native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0))
    a, b = steppers
    assert a.model.permutation is None and not a.overlap_optimizer and not b.overlap_optimizer   # 6000 rows: below the size the overlap pays at
    b.overlap_optimizer = True
    perm = b.model.permutation
    assert torch.equal(a.model.raw[perm], b.model.raw)
    imgs = []
    for st in steppers:
        bt = to_batch(view, DEV); bt.T_to_world = bt.T_to_world.cpu(); bt.rgb_gt = gt
        rgba, _, _, _ = st.forward(bt)
        imgs.append(rgba.clone())
    assert float((imgs[0] - imgs[1]).abs().max()) <= 2e-5
    # forward() left each handle with a cached forward; run two complete steps
    for _ in range(2):
        for st in steppers:
            bt = to_batch(view, DEV); bt.T_to_world = bt.T_to_world.cpu(); bt.rgb_gt = gt
            st.step(bt)
    perm = b.model.permutation
    assert torch.allclose(a.model.raw[perm], b.model.raw, rtol=2e-5, atol=1e-6)
    assert torch.allclose(a.model.features[perm], b.model.features, rtol=2e-5, atol=1e-6)
    assert torch.allclose(a.m48[perm], b.m48, rtol=1e-4, atol=1e-9)
    # move some Gaussians, re-sort: rows and their moments travel together
    with torch.no_grad():
        b.model.raw[:100, 0:3] += 3.0
    tag = b.model.raw[:, 3].clone(); m_tag = b.m12[:, 3].clone(); old_perm = b.model.permutation.clone()
    b.restore_spatial_order()
    new_from_old = torch.argsort(old_perm)[b.model.permutation]   # stored row i now holds what was stored row new_from_old[i]
    assert torch.equal(b.model.raw[:, 3], tag[new_from_old]) and torch.equal(b.m12[:, 3], m_tag[new_from_old])
    bt = to_batch(view, DEV); bt.T_to_world = bt.T_to_world.cpu(); bt.rgb_gt = gt
    loss, _ = b.step(bt)
    assert np.isfinite(float(loss))


def test_selective_adam_inside_the_fused_optimiser_kernel():
    """SelectiveAdam semantics (optimizers.cu:47-117: rows with visibility == 0 are skipped entirely, no bias correction)
    inside k_sh_adam — the one-pass form and the chunked compact form — against the plain per-tensor path
    (gut_adam_step with the visibility mask, itself checked against the closed form in test_selective_adam_semantics)."""
    sc = scenes.scene_c1(3000, 23)
    W, H = 128, 96
    # camera inside the cloud: a good part of the Gaussians is behind it (visibility 0)
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.1, 0.0, 0.0), (1.0, 0.2, 0.1)), fx=110.0)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    variants = dict(plain=dict(fused_sh_adam=False), one_pass=dict(fused_sh_adam=True),
                    chunked=dict(fused_sh_adam=True, fuse_epilogue=False))
    res = {}
    for name, kw in variants.items():
        model = native.NativeGaussianModel(sc, device=DEV)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, selective=True, **kw)
        raw0, feat0 = model.raw.clone(), model.features.clone()
        vis = torch.zeros(model.num_gaussians, dtype=torch.bool, device=DEV)
        for _ in range(2):
            b = to_batch(view, DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
            _, aux = st.step(b)
            vis |= aux["mog_visibility"].reshape(-1) > 0      # visible in either step (a few rows change sides as they move)
        res[name] = dict(raw=model.raw.clone(), feat=model.features.clone(), m48=st.m48.clone(), vis=vis, raw0=raw0, feat0=feat0)
    vis = res["plain"]["vis"]
    assert 200 < int(vis.sum()) < 2800
    for name, r in res.items():
        assert float((r["vis"] != vis).float().mean()) < 1e-2
        vis = vis | r["vis"]
    for name, r in res.items():
        # invisible rows: parameters and moments untouched, bit for bit
        assert torch.equal(r["raw"][~vis], r["raw0"][~vis]) and torch.equal(r["feat"][~vis], r["feat0"][~vis]), name
        assert float(r["m48"][~vis].abs().max()) == 0.0, name
        assert float((r["raw"][vis] - r["raw0"][vis]).abs().max()) > 0
    for name in ("one_pass", "chunked"):
        assert rel_l2(res[name]["raw"].cpu().numpy(), res["plain"]["raw"].cpu().numpy()) <= 1e-5, name
        assert rel_l2(res[name]["feat"].cpu().numpy(), res["plain"]["feat"].cpu().numpy()) <= 1e-5, name
        assert rel_l2(res[name]["m48"].cpu().numpy(), res["plain"]["m48"].cpu().numpy()) <= 1e-4, name


def test_overlap_probe_keeps_the_faster_optimiser_form(monkeypatch):
    """With the overlap on by default NativeTrainStep times steps 2..9 alternately with and without it and keeps the form whose
    best sample is faster; forced settings are never probed.  (Made applicable to a small scene by lowering the size gate.)"""
    sc = scenes.scene_c1(4000, 9)
    W, H = 96, 64
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.2, 0.0, -3.5), (0, 0, 0)), fx=90.0)
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
    forced = native.NativeTrainStep(model, gut.Tracer({"render": {}}), overlap_optimizer=True)
    assert forced._overlap_probe is None
    model2 = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
    monkeypatch.setattr(native.NativeTrainStep, "OVERLAP_MIN_GAUSSIANS", 1000)
    st = native.NativeTrainStep(model2, gut.Tracer({"render": {}}))
    assert st.overlap_optimizer and st._overlap_probe is not None
    for _ in range(14):
        b = to_batch(view, DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
        loss, _ = st.step(b)
        torch.cuda.synchronize()
    p = st._overlap_probe
    assert p["done"] and len(p["on"]) == 4 and len(p["off"]) == 4 and p["ms_on"] > 0 and p["ms_off"] > 0
    assert st.overlap_optimizer == (p["ms_on"] <= p["ms_off"])
    assert np.isfinite(float(loss))


def test_train_step_with_the_selective_adam_option():
    """train.TrainStep(optimizer_type="selective_adam") = the reference's `optimizer.type: selective_adam` (model.py:512, trainer.py:
    747-749): rows the view did not see keep parameters and moments bit for bit; rows it saw move, on the FIRST step (zero moments),
    (1 - beta1) / sqrt(1 - beta2) = 3.1623 times as far as torch.optim.Adam moves them — the reference's SelectiveAdam has no bias
    correction, Adam's first step is lr * sign(g)."""
    train_mod = importlib.import_module("3dgrut_amd.train")
    model_mod = importlib.import_module("3dgrut_amd.model")
    sc = scenes.scene_c1(6000, 41)
    W, H = 96, 72
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.0, 0.0, 0.0), (1, 0, 0)), fx=90.0)
    b = to_batch(view, DEV)
    b.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    steppers = {}
    for kind in ("adam", "selective_adam"):
        model = model_mod.GaussianModel(sc, device=DEV, sh_degree=3)
        steppers[kind] = train_mod.TrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, optimizer_type=kind, fused_adam=False)
    start = {n: p.detach().clone() for n, p in steppers["adam"].model.named_parameters()}
    outs = {k: st.step(b)[1] for k, st in steppers.items()}
    vis = outs["selective_adam"]["mog_visibility"].bool().squeeze()
    assert 100 < int(vis.sum()) < 6000
    pa, ps = dict(steppers["adam"].model.named_parameters()), dict(steppers["selective_adam"].model.named_parameters())
    for name, p0 in start.items():
        assert torch.equal(ps[name][~vis], p0[~vis]), name
        d_sel, d_adam = (ps[name][vis] - p0[vis]).double(), (pa[name][vis] - p0[vis]).double()
        moved = d_adam.abs() > 1e-3 * d_adam.abs().max()          # (steps below the parameter's ulp say nothing about the ratio)
        assert int(moved.sum()) > 100, name
        ratio = d_sel[moved] / d_adam[moved]
        # (gradients around eps = 1e-15 — Gaussians a ray barely touched — sit in the eps-dominated regime of both formulas: a few percent of the scale rows)
        assert float(((ratio - 0.1 / 0.001 ** 0.5).abs() < 2e-2).double().mean()) > 0.95, name
        assert float(ratio.min()) > 0.0 and float(ratio.max()) < 3.17, name
        st = steppers["selective_adam"].optimizer.state[ps[name]]
        assert not st["exp_avg"][~vis].any() and not st["exp_avg_sq"][~vis].any()
    with pytest.raises(ValueError):
        train_mod.TrainStep(steppers["adam"].model, gut.Tracer({"render": {}}), optimizer_type="lion")


def test_scratch_buffers_can_be_moved_between_steps():
    """GUT_OPT_DEBUG_REPLACE_SCRATCH (the developer probe behind tools/scratch_placement.py): every scratch buffer of the handle moves
    to a fresh allocation between two train steps, contents kept — the library holds no stale pointer to any of them: the next
    steps run, and the trainer ends where an undisturbed one ends (up to the float-atomic order of the backward)."""
    sc = scenes.scene_c1(30000, 17)
    W, H = 128, 96
    views = [make_view("pinhole", W, H, cams.look_at_c2w((0.2 * k, 0.1, -3.0), (0, 0, 0)), fx=110.0) for k in range(3)]
    gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(9)).to(DEV)
    ends = []
    for disturb in (False, True):
        model = native.NativeGaussianModel(sc, device=DEV, spatial_order=True)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, overlap_optimizer=True)
        for k in range(6):
            b = to_batch(views[k % 3], DEV); b.T_to_world = b.T_to_world.cpu(); b.rgb_gt = gt
            st.step(b)
            if disturb and k in (1, 3):
                for idx in range(20):
                    st.raster.debug_replace_scratch(idx)
        st.sync_moments()
        ends.append((model.raw.clone(), model.features.clone(), st.m48.clone()))
    with pytest.raises(RuntimeError, match="GUT_OPT_DEBUG_REPLACE_SCRATCH"):
        st.raster.debug_replace_scratch(20)
    for a, b in zip(*ends):
        assert bool(torch.isfinite(b).all()) and rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= 1e-4
