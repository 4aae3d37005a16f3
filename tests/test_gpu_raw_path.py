"""The product default render path — Tracer.raw_parameters: the model's pre-activation tensors go to gut_trace_raw_model_fields, the
library activates them in-kernel and K8 returns raw-parameter gradients — against the CPU oracle PER ROW, on the cases the rest of the
suite only gives the activated path: rolling shutter x camera model, SH degrees 0 - 2, two generalised kernels, fuzz draws with the
raw tensors re-drawn wide (logits -12 ... 8, log-scale offsets down to -3 and up to +3 where the scene stays renderable, quaternion
norms 1e-3 ... 1e3), N = 1, 63, 1001, and the sorted (k-buffer) variant at K = 4.

The oracle is fed the rows the kernels read (debug_buffer("packed_rows"), pad column zeroed).  Forward: integer buffers and projection
floats bit for bit, the image by check_colour_outliers, the packed rows against reference_step.activate element by element.  Backward:
the oracle's [N,12] gradient is chained to the raw parameters by reference_step.chain in float64; its noise and flip budget, one scalar
per row and block, scale by the operator norm of that block's Jacobian (y (1 - y), 1 / |q|, max_k exp(s_k), 1); every block then goes
through tests.common.check_gradient_rows with the shared constants.  Rows without a tile have exactly zero gradient in all six tensors.
The chain rule below normalize's clamp (|q| < 1e-12) is not a number to compare (torch: g / 1e-12, the kernels: the projection) and is
not drawn."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import reference_step as R
from tests.common import (FISHEYE_DIST, K_ACT, K_ADAM, K_CHAIN, ROW_ABS, ROW_FLIP, ROW_FLIP_BOUND, ROW_NOISE, ROW_REL, cams, check_colour_outliers,
                          K_MOMENT, check_gradient_rows, make_view, scenes, to_batch)
from tests.test_gpu_fuzz import _case
from tests.test_gpu_parity import CASES, gut_model

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
oracle = importlib.import_module("oracle.oracle")
pose_mod = importlib.import_module("3dgrut_amd.pose")
DEV = "cuda:0"
BLOCKS = (("positions", slice(0, 3)), ("density", slice(3, 4)), ("rotation", slice(4, 8)), ("scale", slice(8, 11)))


def _redraw_wide(model, seed):
    """The model's raw tensors re-drawn wider than any scene builder gives them: what MCMC's opacity regulariser, densification
    and an unconstrained quaternion leave behind."""
    rng = np.random.default_rng(seed)
    n = model.positions.shape[0]
    with torch.no_grad():
        model.density.copy_(torch.as_tensor(rng.uniform(-12.0, 8.0, (n, 1)).astype(np.float32)))
        s = model.scale.detach().cpu().numpy().astype(np.float64)
        # offsets of up to +-3 where the scene allows: no axis is taken above 0.5 scene units (the frame stays renderable on the CPU) or
        # below 2e-4, the smallest scale of the fuzz sweep's own deliberately ill-conditioned draws — below it the ray origin in the
        # particle's canonical space exceeds 1e4 and fp32 has no digits left in ANY formulation (tests/test_gpu_fuzz.py)
        s = np.clip(s + rng.uniform(-3.0, 3.0, (n, 1)), np.minimum(s, math.log(2e-4)), np.maximum(s, math.log(0.5)))
        model.scale.copy_(torch.as_tensor(s.astype(np.float32)))
        model.rotation.mul_(torch.as_tensor((10.0 ** rng.uniform(-3.0, 3.0, (n, 1))).astype(np.float32), device=model.rotation.device))


def _raw12(model):
    with torch.no_grad():
        return torch.cat([model.positions, model.density, model.rotation, model.scale, torch.zeros_like(model.density)], 1).cpu().numpy()


def _check_chained_rows(label, grads, raw, dens_g, sph_g, budget, sh, tiles_count):
    """The six gradient tensors of the raw path, per row, against a gradient w.r.t. the ACTIVATED rows (dens_g [N,12], sph_g [N,48],
    float64) chained to the raw parameters by reference_step.chain.  budget [N,10]: oracle.backward's flip budget and noise per row
    and block; each is one scalar per row, so it scales by the operator norm of that block's Jacobian.  check_gradient_rows' absolute
    term is chained the same way, per row: ROW_ABS x (the scale of the ACTIVATED block) x the row's operator norm — with quaternion
    norms over six decades a single scale of the chained block (its 99th-percentile row) would leave every row with a large |q| or
    a saturated opacity unchecked.  It enters through the noise argument (divided by ROW_NOISE: factor one), with abs_tol = 0; so does
    the chain rule's own fp32 tolerance (reference_step.chain, K_CHAIN).  Rows without a tile: exactly zero in all six tensors."""
    graw, ccond = R.chain(raw, dens_g)
    norms = R.chain_operator_norms(raw)
    cb = ccond.bound(K_CHAIN)
    worst = {}
    for j, (name, sl) in enumerate(BLOCKS):
        nr = np.linalg.norm(dens_g[:, sl], axis=1)
        scale_act = float(np.quantile(nr[nr > 0], 0.99)) if (nr > 0).any() else 0.0     # check_gradient_rows' definition, on the activated block
        extra = (ROW_ABS * scale_act * norms[:, j] + np.linalg.norm(cb[:, sl], axis=1)) / ROW_NOISE
        rep = check_gradient_rows(grads[name], graw[:, sl], f"{label}/raw/{name}", budget[:, j] * norms[:, j],
                                  budget[:, 5 + j] * norms[:, j] + extra, abs_tol=0.0)
        worst[name] = rep["worst_row_vs_full_bound"]
    nc = (sh + 1) ** 2
    for name, sl, factor in (("features_albedo", slice(0, 3), math.sqrt(1.0 / (4 * math.pi))),
                             ("features_specular", slice(3, 48), math.sqrt((nc - 1) / (4 * math.pi)))):
        if not sph_g[:, sl].any():
            assert not grads[name].any(), (label, name, "the reference gradient is exactly zero")
            continue
        rep = check_gradient_rows(grads[name], sph_g[:, sl], f"{label}/raw/{name}", budget[:, 4] * factor, budget[:, 9] * factor)
        worst[name] = rep["worst_row_vs_full_bound"]
    no_tile = np.asarray(tiles_count) == 0
    for k, g in grads.items():
        assert not g[no_tile].any(), (label, k, "a row without a tile has a gradient")
    return worst


def _check_raw_path(label, model, view, sh, rgba_grad, ocam=None, sensor_edit=None, tq_end=None, conf=None, params=None):
    """One forward + backward through the raw path, every check of the module docstring.  Returns the worst row ratios it printed."""
    W, H = view["W"], view["H"]
    ocam = ocam or view["oracle_cam"]
    tracer = gut.Tracer({"render": dict(conf or {})})
    tracer.raw_parameters = True
    batch = to_batch(view, DEV)
    if sensor_edit is None and tq_end is None:
        out = tracer.render(model, batch, train=True)
        rgb, opacity, hits = out["pred_rgb"][0], out["pred_opacity"][0], out["hits_count"][0]
    else:   # rolling shutter: Tracer.render gives both ends of the exposure the same pose, so the autograd function is called as it calls it
        sensor, poses = gut.Tracer.create_camera_parameters(batch)
        sensor_edit(sensor)
        poses.T_world_sensors[1] = tq_end
        rgba, _, hits, _ = gut.Tracer._Autograd.apply(
            tracer.tracer_wrapper, 0, model.n_active_features, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(),
            model.positions.contiguous(), model.rotation.contiguous(), model.scale.contiguous(), model.density.contiguous(),
            model.get_features_albedo().contiguous(), sensor, poses, model.get_features_specular().contiguous(), True)
        rgb, opacity = rgba[..., :3], rgba[..., 3:]
    rg = torch.as_tensor(rgba_grad, device=DEV)
    ((rgb * rg[..., :3]).sum() + (opacity * rg[..., 3:]).sum()).backward()
    r = tracer.tracer_wrapper
    raw = _raw12(model)
    n = raw.shape[0]
    assert (np.linalg.norm(raw[:, 4:8].astype(np.float64), axis=1) >= 1e-12).all()
    # ---- forward
    rows = r.debug_buffer("packed_rows").reshape(-1, 12).cpu().numpy()
    aref, acond = R.activate(raw)
    aerr = np.abs(rows.astype(np.float64) - aref)
    abound = acond.bound(K_ACT)
    assert (aerr <= abound).all(), (label, "packed_rows", np.argwhere(aerr > abound)[:3])
    d12 = rows.copy(); d12[:, 11] = 0.0
    sph = model.get_features().detach().cpu().numpy()
    ref = oracle.forward(ocam, W, H, d12, sph, view["ro"], view["rd"], sh_degree=sh, params=params)
    for key in ("tiles_count", "tiles_offset", "unsorted_ids", "sorted_ids"):
        assert np.array_equal(r.debug_buffer(key).cpu().numpy().view(np.uint32), ref[key]), (label, key)
    assert np.array_equal(r.debug_buffer("sorted_keys").cpu().numpy().view(np.uint64), ref["sorted_keys"]), label
    for key in ("proj_pos", "conic_opacity", "extent", "depth", "feat"):
        got = r.debug_buffer(key).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.ascontiguousarray(ref[key]).reshape(-1).view(np.uint32)), (label, key)
    grads = {k: (getattr(model, k).grad.detach().cpu().numpy() if getattr(model, k).grad is not None else None)
             for k in ("positions", "density", "rotation", "scale", "features_albedo", "features_specular")}
    rgba_np = np.concatenate([rgb.detach().cpu().numpy(), opacity.detach().cpu().numpy()], -1)
    if ref["M"] == 0:
        assert np.abs(rgba_np - ref["rgba"]).max() == 0.0
        for k, g in grads.items():
            assert g is None or not g.any(), (label, k)
        print(f"[raw path {label}] N={n}: no intersections, image and all six gradients exactly zero")
        return {}
    margins, pixel_budget = oracle.render_margins(ocam, ref, params=params, budget_bound=ROW_FLIP_BOUND)
    check_colour_outliers(rgba_np, hits.detach().cpu().numpy(), ref, margins, label=f"{label}/raw", budget=pixel_budget)
    # ---- backward, per row
    dens_g, sph_g, _, budget = oracle.backward(ocam, ref, rgba_grad, np.zeros((H, W, 1), np.float32), params=params, flip_bound=ROW_FLIP_BOUND)
    worst = _check_chained_rows(label, grads, raw, dens_g, sph_g, budget, sh, ref["tiles_count"])
    no_tile = ref["tiles_count"] == 0
    print(f"[raw path {label}] N={n} M={ref['M']} rows without a tile {int(no_tile.sum())}; worst row vs bound {worst}; "
          f"packed rows worst {float((aerr / np.maximum(abound, 1e-300)).max()):.3f} of bound")
    return worst


def _grad_image(H, W, seed):
    return np.random.default_rng(seed).normal(size=(H, W, 4)).astype(np.float32)


@pytest.mark.parametrize("shutter", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["pinhole", "fisheye_distorted"])
def test_raw_path_with_a_rolling_shutter(shutter, kind):
    """test_rolling_shutter_projection's grid (distinct start / end poses) through the raw path, forward and backward."""
    sc = scenes.scene_c1(700, 40 + shutter)
    W, H = 96, 80
    distortion = FISHEYE_DIST if kind == "fisheye_distorted" else None
    vkind = "fisheye" if distortion else kind
    view = make_view(vkind, W, H, cams.look_at_c2w((0.1, 0.0, -3.0 if vkind == "pinhole" else -1.6), (0, 0, 0)), fx=90 if vkind == "pinhole" else None,
                     distortion=distortion)
    end_c2w = cams.look_at_c2w((0.25, -0.1, -2.9 if vkind == "pinhole" else -1.55), (0.05, 0.0, 0.0))
    tq_end = pose_mod.sensor_pose_from_c2w(end_c2w).T_world_sensors[0]
    ocam = dict(view["oracle_cam"], shutter=shutter, pose_end=tq_end)
    model = gut_model(sc, 3)
    _redraw_wide(model, 500 + shutter)

    def edit(sensor):
        sensor.cam.shutter = shutter

    _check_raw_path(f"shutter {shutter} {kind}", model, view, 3, _grad_image(H, W, shutter), ocam=ocam, sensor_edit=edit, tq_end=tq_end)


@pytest.mark.parametrize("sh", [0, 1, 2])
@pytest.mark.parametrize("case", ["c1_pinhole_128", "fisheye_distorted"])
def test_raw_path_at_lower_sh_degrees(case, sh):
    mk, kind, W, H, (eye, tgt), kw = CASES[case]
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    model = gut_model(mk(), sh)
    assert model.n_active_features == sh
    _redraw_wide(model, 600 + sh)
    _check_raw_path(f"{case} sh {sh}", model, view, sh, _grad_image(H, W, 10 + sh))


@pytest.mark.parametrize("degree", [1, 4])
def test_raw_path_with_generalised_kernels(degree):
    mk, kind, W, H, (eye, tgt), kw = CASES["ragged_100x70"]
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    model = gut_model(mk(), 3)
    _redraw_wide(model, 700 + degree)
    prm = oracle.default_params()
    prm.kernel_degree = degree
    _check_raw_path(f"kernel degree {degree}", model, view, 3, _grad_image(H, W, 20 + degree), conf={"particle_kernel_degree": degree}, params=prm)


@pytest.mark.parametrize("seed", range(8))
def test_raw_path_on_fuzz_draws(seed):
    sc, view, W, H, sh, rng = _case(seed)
    model = gut_model(sc, sh)
    _redraw_wide(model, 800 + seed)
    _check_raw_path(f"fuzz {seed}", model, view, sh, rng.normal(size=(H, W, 4)).astype(np.float32))


@pytest.mark.parametrize("n", [1, 63, 1001])
def test_raw_path_row_counts(n):
    sc = scenes.scene_c1(n, 90 + n)
    if n == 1:
        sc["positions"][:] = (0.05, -0.02, 0.1)
    view = make_view("pinhole", 80, 64, cams.look_at_c2w((0.1, 0.2, -3.0), (0, 0, 0)), fx=70)
    model = gut_model(sc, 3)
    _redraw_wide(model, 900 + n)
    if n == 1:   # one opaque, anisotropic Gaussian in front of the camera: every block of its row has a gradient that is not a cancellation residue
        with torch.no_grad():
            model.density.fill_(2.0)
            model.scale.copy_(torch.log(torch.tensor([[0.3, 0.1, 0.05]])))
    w = _check_raw_path(f"N={n}", model, view, 3, _grad_image(64, 80, n))
    assert w, "the case rendered nothing: it tests nothing"


def test_raw_path_sorted_variant():
    """The sorted (k-buffer) variant through the raw path, K = 4, forward and backward.  Packed rows element by element, binning
    buffers bit for bit; image against oracle_render_kbuffer PER PIXEL with check_colour_outliers' quantitative form (every pixel within
    COLOUR_TOL + PIX_FLIP x its own flip budget, hit count within its own count of flip-prone decisions): the k-buffer composites the
    hits the unsorted compositor would, tested against the same thresholds, so the oracle's per-pixel margins and budgets of those
    decisions apply; what they do not model — two hits whose distances agree to an ulp changing places — moves a pixel by the
    difference of two adjacent contributions, which the budget of either hit covers.
    Backward: float64 autograd through oracle/per_ray_torch.composite_ordered on the order the C oracle recorded (the exact derivative:
    sorted_reference_backward off, as tests/test_gpu_parity.py::test_sorted_variant_backward), chained to the raw tensors and compared
    per row by _check_chained_rows.  The float64 reference carries no noise of its own; the GPU's fp32 noise and the flips of its
    hit / no-hit decisions against the oracle's are those of the same per-hit formulas and thresholds as in the unsorted compositor,
    so the per-row noise and flip budget are oracle.backward's for the same lists and the same image gradient (one scalar per row and
    block, an estimate of magnitude that does not depend on the order of composition)."""
    prt = importlib.import_module("oracle.per_ray_torch")
    K = 4
    mk, kind, W, H, (eye, tgt), kw = CASES["c1_pinhole_128"]
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    model = gut_model(mk(), 3)
    _redraw_wide(model, 1000)
    tracer = gut.Tracer({"render": {"splat": {"k_buffer_size": K, "sorted_reference_backward": False}}})
    tracer.raw_parameters = True
    rgba_grad = _grad_image(H, W, 44)
    out = tracer.render(model, to_batch(view, DEV), train=True)
    rg = torch.as_tensor(rgba_grad, device=DEV)
    ((out["pred_rgb"][0] * rg[..., :3]).sum() + (out["pred_opacity"][0] * rg[..., 3:]).sum()).backward()
    r = tracer.tracer_wrapper
    raw = _raw12(model)
    rows = r.debug_buffer("packed_rows").reshape(-1, 12).cpu().numpy()
    aref, acond = R.activate(raw)
    assert (np.abs(rows.astype(np.float64) - aref) <= acond.bound(K_ACT)).all()
    d12 = rows.copy(); d12[:, 11] = 0.0
    sph = model.get_features().detach().cpu().numpy()
    fwd = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    for key in ("tiles_count", "tiles_offset", "sorted_ids"):
        assert np.array_equal(r.debug_buffer(key).cpu().numpy().view(np.uint32), fwd[key]), key
    for key in ("proj_pos", "conic_opacity", "extent", "depth", "feat"):
        assert np.array_equal(r.debug_buffer(key).cpu().numpy().view(np.uint32), np.ascontiguousarray(fwd[key]).reshape(-1).view(np.uint32)), key
    max_order = int(fwd["hits"].max()) + 64
    ref = oracle.render_kbuffer(view["oracle_cam"], fwd, K=K, max_order=max_order)
    margins, pixel_budget = oracle.render_margins(view["oracle_cam"], fwd, budget_bound=ROW_FLIP_BOUND)
    rgba_np = np.concatenate([out["pred_rgb"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1)
    check_colour_outliers(rgba_np, out["hits_count"][0].detach().cpu().numpy(), dict(rgba=ref["rgba"], hits=ref["hits"]), margins,
                          label="sorted K=4/raw", budget=pixel_budget)
    L = max(int(ref["order_count"].max()), 1)
    params = dict(positions=d12[:, 0:3], density=d12[:, 3:4], rotation=d12[:, 4:8], scale=d12[:, 8:11], features=sph)
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    rgba64, _ = prt.composite_ordered(params, view["tq"], W, H, view["ro"], view["rd"], ref["order_ids"][:, :L], ref["order_count"])
    assert np.abs(rgba64.detach().numpy().reshape(H, W, 4) - ref["rgba"]).max() <= 5e-5
    (rgba64 * torch.tensor(rgba_grad.reshape(-1, 4), dtype=torch.float64)).sum().backward()
    dens_g = np.zeros((d12.shape[0], 12))
    dens_g[:, 0:3] = params["positions"].grad.numpy(); dens_g[:, 3:4] = params["density"].grad.numpy()
    dens_g[:, 4:8] = params["rotation"].grad.numpy(); dens_g[:, 8:11] = params["scale"].grad.numpy()
    sph_g = params["features"].grad.numpy()
    _, _, _, budget = oracle.backward(view["oracle_cam"], fwd, rgba_grad, np.zeros((H, W, 1), np.float32), flip_bound=ROW_FLIP_BOUND)
    grads = {k: getattr(model, k).grad.detach().cpu().numpy() for k in ("positions", "density", "rotation", "scale", "features_albedo", "features_specular")}
    worst = _check_chained_rows("sorted K=4", grads, raw, dens_g, sph_g, budget, 3, fwd["tiles_count"])
    print(f"[raw path sorted K=4] N={raw.shape[0]} M={fwd['M']}; worst row vs bound {worst}")


# ---------------------------------------------------------------------------------------------------------------------------------
# One native step (one-pass form: chain rule + SH gradient + Adam in one kernel, straight from the handle's gradient rows) against the
# oracle, per element
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_raw_gradient(tn, mn, view, batch, sh):
    """The oracle's gradient w.r.t. the raw rows and the [N,48] features at the trainer's CURRENT parameters, with its per-element
    uncertainty: the image gradient is the float64 autograd gradient of train.photometric_loss_torch at the image a forward-only
    render returned (tests/test_gpu_losses.py ties the fused loss kernel's gradient to it to 1e-4); the row terms are
    check_gradient_rows' (ROW_REL |row| + ROW_ABS scale + ROW_NOISE noise + ROW_FLIP budget), chained with the Jacobians' norms."""
    train = importlib.import_module("3dgrut_amd.train")
    W, H = view["W"], view["H"]
    rgba = tn.forward(batch)[0].detach().clone()
    leaf = rgba.double().requires_grad_(True)
    train.photometric_loss_torch(leaf[..., :3].unsqueeze(0), batch.rgb_gt.double()).backward()
    rgba_grad = leaf.grad.float().cpu().numpy()
    raw = mn.raw.detach().cpu().numpy()
    d12 = tn.activate().detach().cpu().numpy().reshape(-1, 12).copy(); d12[:, 11] = 0.0
    ref = oracle.forward(view["oracle_cam"], W, H, d12, mn.features.cpu().numpy(), view["ro"], view["rd"], sh_degree=sh)
    dens_g, sph_g, _, budget = oracle.backward(view["oracle_cam"], ref, rgba_grad, np.zeros((H, W, 1), np.float32), flip_bound=ROW_FLIP_BOUND)
    graw, ccond = R.chain(raw, dens_g)
    norms = R.chain_operator_norms(raw)
    unc12 = ccond.bound(K_CHAIN)
    for j, (name, sl) in enumerate(BLOCKS):
        nr = np.linalg.norm(graw[:, sl], axis=1)
        na = np.linalg.norm(dens_g[:, sl], axis=1)
        # (check_gradient_rows' own definition of a block's scale, on the activated block, chained per row as in _check_chained_rows:
        #  no row is excluded by it)
        scale = float(np.quantile(na[na > 0], 0.99)) if (na > 0).any() else 0.0
        row = (ROW_REL + 1e-4) * nr + (ROW_ABS * scale + ROW_NOISE * budget[:, 5 + j] + ROW_FLIP * budget[:, j]) * norms[:, j]
        unc12[:, sl] += row[:, None]
    y = math.sqrt((sh + 1) ** 2 / (4 * math.pi))
    nr = np.linalg.norm(sph_g, axis=1)
    scale = float(np.quantile(nr[nr > 0], 0.99)) if (nr > 0).any() else 0.0
    unc48 = np.repeat(((ROW_REL + 1e-4) * nr + ROW_ABS * scale + (ROW_NOISE * budget[:, 9] + ROW_FLIP * budget[:, 4]) * y)[:, None], 48, 1)
    unc48[:, 3 * (sh + 1) ** 2:] = 0.0
    return graw, unc12, sph_g, unc48


@pytest.mark.parametrize("case", ["c1_pinhole_128", "fisheye_distorted"])
def test_one_pass_native_step_against_the_oracle_per_element(case):
    """NativeTrainStep.step() (fuse_epilogue: gut_optimize_after_bwd reads the handle's gradient rows, chains them to the raw
    parameters, rebuilds the SH gradient and applies Adam in one kernel), fresh moments, all learning-rate columns different.
    Step 1 (zero moments: the update is -lr g / (|g| + eps), +-lr wherever g != 0): on every element whose oracle gradient exceeds
    its own uncertainty the sign is the gradient's and the size is lr; rows to which the oracle gives an exactly zero gradient keep
    their bits and their zero moments, and both moments equal (1 - beta) g and (1 - beta) g^2 within the gradient's uncertainty.  Step 2 on the same view (non-zero moments: magnitude-sensitive): raw and features against
    reference_step.step fed the kernels' own moments and the oracle's gradient at the parameters step 1 left, every element within
    the Adam bound with the gradient's uncertainty pushed through it."""
    native = importlib.import_module("3dgrut_amd.native")
    mk, kind, W, H, (eye, tgt), kw = CASES[case]
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    mn = native.NativeGaussianModel(mk(), device=DEV)
    tn = native.NativeTrainStep(mn, gut.Tracer({"render": {}}), scene_extent=1.0, fused_sh_adam=True, fuse_epilogue=True)
    tn.lr12[:] = R.lr_ladder(12, 1e-5, 2e-2)
    tn.lr48[:] = R.lr_ladder(48, 2e-5, 1e-2)
    sh = mn.n_active_features
    b1, b2 = tn.betas
    eps = float(np.float32(tn.eps))
    # ---- step 1
    raw0, f0 = mn.raw.detach().cpu().numpy().copy(), mn.features.detach().cpu().numpy().copy()
    g12, u12, g48, u48 = _oracle_raw_gradient(tn, mn, view, batch, sh)
    tn.step(batch)
    torch.cuda.synchronize()
    raw1, f1 = mn.raw.detach().cpu().numpy().copy(), mn.features.detach().cpu().numpy().copy()
    checked = 0
    for name, p0, p1, g, u, lr in (("raw", raw0[:, :11], raw1[:, :11], g12[:, :11], u12[:, :11], tn.lr12[:11]), ("features", f0, f1, g48, u48, tn.lr48)):
        dp = p1.astype(np.float64) - p0.astype(np.float64)
        sure = np.abs(g) > u
        lrs = np.broadcast_to(lr.astype(np.float64)[None, :], g.shape)
        assert (np.sign(dp[sure]) == -np.sign(g[sure])).all(), (case, name, "an update has the wrong sign", np.argwhere(sure & (np.sign(dp) != -np.sign(g)))[:3])
        lo = lrs * (np.abs(g) - u) / (np.abs(g) - u + eps)
        slack = K_ADAM * R.EPS * lrs + 0.5 * R.ulp32_up(np.abs(p0) + lrs) + 0.5 * R.ulp32_up(p0)
        bad = sure & ((np.abs(dp) > lrs + slack) | (np.abs(dp) < lo - slack))
        assert not bad.any(), (case, name, "an update is not lr in size", np.argwhere(bad)[:3], dp[bad][:3], lrs[bad][:3])
        checked += int(sure.sum())
        zero_rows = ~g.any(1) if name == "features" else ~g12[:, :11].any(1)
        assert np.array_equal(p1[zero_rows].view(np.uint32), p0[zero_rows].view(np.uint32)), (case, name, "a row without a gradient moved")
    zero12, zero48 = ~g12[:, :11].any(1), ~g48.any(1)
    assert not tn.m12.cpu().numpy()[zero12].any() and not tn.v12.cpu().numpy()[zero12].any()
    assert not tn.m48.cpu().numpy()[zero48].any() and not tn.v48.cpu().numpy()[zero48].any()
    assert checked > 2000, checked
    # ... and the moments step 1 left, every element: (1 - beta) g and (1 - beta) g^2 with the gradient's uncertainty pushed through
    zeros12, zeros48 = np.zeros_like(raw0), np.zeros_like(f0)
    ref1 = R.step(raw0, zeros12, zeros12, f0, zeros48, zeros48, g12, None, None, sh, 1.0, tn.lr12, tn.lr48, b1, b2, tn.eps, 1, g12_unc=u12, g48=g48, g48_unc=u48)
    tn.sync_moments()
    for name, got in (("m12", tn.m12), ("v12", tn.v12), ("m48", tn.m48), ("v48", tn.v48)):
        val, cond = ref1[name]
        cols = slice(0, 11) if name.endswith("12") else slice(0, 48)
        err, bound = np.abs(got.detach().cpu().numpy().astype(np.float64) - val)[:, cols], cond.bound(K_MOMENT)[:, cols]
        assert (err <= bound).all(), (case, name, "after step 1", int((err > bound).sum()), np.argwhere(err > bound)[:3])
    # ---- step 2: the kernels' own state after step 1, the oracle's gradient there
    m12, v12, m48, v48 = (t.detach().cpu().numpy().copy() for t in (tn.m12, tn.v12, tn.m48, tn.v48))   # (synced above)
    g12, u12, g48, u48 = _oracle_raw_gradient(tn, mn, view, batch, sh)
    tn.step(batch)
    torch.cuda.synchronize()
    ref = R.step(raw1, m12, v12, f1, m48, v48, g12, None, None, sh, 1.0, tn.lr12, tn.lr48, b1, b2, tn.eps, 2, g12_unc=u12, g48=g48, g48_unc=u48)
    worst = {}
    for name, got, key in (("raw", mn.raw, "raw12"), ("features", mn.features, "sh48")):
        val, cond = ref[key]
        got = got.detach().cpu().numpy().astype(np.float64)
        cols = slice(0, 11) if name == "raw" else slice(0, 48)
        err, bound = np.abs(got - val)[:, cols], cond.bound(K_ADAM)[:, cols]
        assert (err <= bound).all(), (case, name, int((err > bound).sum()), np.argwhere(err > bound)[:3], float((err / np.maximum(bound, 1e-300)).max()))
        moved = np.abs(val - (raw1 if name == "raw" else f1))[:, cols]
        worst[name] = (float((err / np.maximum(bound, 1e-300)).max()), float(np.median(bound[moved > 0] / moved[moved > 0])))
    # the moments after step 2 (brought up to date first: a wave that could not receive a gradient keeps stale stored moments), every
    # element: K_MOMENT + 2, the two extra roundings being the lazy decay's table entry and its product with the stored moment
    tn.sync_moments()
    for name, got in (("m12", tn.m12), ("v12", tn.v12), ("m48", tn.m48), ("v48", tn.v48)):
        val, cond = ref[name]
        cols = slice(0, 11) if name.endswith("12") else slice(0, 48)
        err, bound = np.abs(got.detach().cpu().numpy().astype(np.float64) - val)[:, cols], cond.bound(K_MOMENT + 2)[:, cols]
        assert (err <= bound).all(), (case, name, int((err > bound).sum()), np.argwhere(err > bound)[:3], float((err / np.maximum(bound, 1e-300)).max()))
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[native step {case}] step 1: {checked} elements with a certain gradient moved by -sign(g) lr; step 2: (worst error / bound, "
          f"median bound / |update|) {worst}")
