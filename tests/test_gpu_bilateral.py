"""The bilateral grids of DESIGN.md §21 on the GPU: the slice, the image gradient, the grid gradient, the TV term and the Adam step
bit for bit against the float32 restatement of tests/bilateral_reference.py (its cases and their preconditions are checked in
tests/test_cpu_bilateral.py); apply() under autograd against the float64 definition; one fused step against the torch branch; a
stepper with the switch and no grid; the recovery of known grids with the Gaussians frozen; a trainer run with its resume."""
import copy
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import bilateral_reference as br
from tests.common import rel_l2, scenes
from tests.synthetic_colmap import load_scene, write_synthetic_colmap
from tests.test_gpu_background_training import _batch

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
_capi = importlib.import_module("3dgrut_amd._capi")
native = importlib.import_module("3dgrut_amd.native")
losses = importlib.import_module("3dgrut_amd.losses")
bilateral = importlib.import_module("3dgrut_amd.bilateral")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
DEV = "cuda:0"
NAN = float("nan")
F = np.float32


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _same_bits(a, b):
    """Bit for bit, a NaN for a NaN (the payload of a NaN is not part of the contract)."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _record(grid):
    L, Gh, Gw = (int(n) for n in grid.shape[1:])
    return _capi.GutBilateralGrid(grid.data_ptr(), L, Gh, Gw)


def _bg(background):
    """(plane pointer or None, constant, the tensor to keep alive)."""
    if np.ndim(background) == 0:
        return None, float(background), None
    t = _dev(background)
    return t.data_ptr(), 0.0, t


def _slice(c):
    """gut_bilateral_slice into a NaN-filled image."""
    rgba, grid = _dev(c["rgba"]), _dev(c["grid"])
    H, W = rgba.shape[:2]
    plane, constant, keep = _bg(c["background"])
    out = torch.full((H, W, 4), NAN, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(_capi.load().gut_bilateral_slice(C.c_void_p(stream), H, W, rgba.data_ptr(), plane, constant, C.byref(_record(grid)),
                                                 out.data_ptr()), "bilateral_slice")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _backward(c, out_grad, lambda_tv=0.0):
    """gut_bilateral_backward into NaN-filled gradients, from a workspace filled with -1."""
    lib = _capi.load()
    rgba, grid, og = _dev(c["rgba"]), _dev(c["grid"]), _dev(out_grad)
    H, W = rgba.shape[:2]
    plane, constant, keep = _bg(c["background"])
    rec = _record(grid)
    ws = torch.full(((lib.gut_bilateral_workspace_bytes(rec.levels, rec.rows, rec.columns) + 7) // 8,), -1, dtype=torch.int64, device=DEV)
    rgba_grad = torch.full((H, W, 4), NAN, dtype=torch.float32, device=DEV)
    grid_grad = torch.full(tuple(grid.shape), NAN, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.gut_bilateral_backward(C.c_void_p(stream), H, W, rgba.data_ptr(), plane, constant, C.byref(rec), og.data_ptr(),
                                           float(lambda_tv), ws.data_ptr(), rgba_grad.data_ptr(), grid_grad.data_ptr()), "bilateral_backward")
    torch.cuda.synchronize()
    return rgba_grad.cpu().numpy(), grid_grad.cpu().numpy()


# ---- 1. the kernels alone, bit for bit ----
@pytest.mark.parametrize("name", list(br.CASES))
def test_slice_bit_for_bit(name):
    c = br.case(name)
    got = _slice(c)
    assert _same_bits(got, br.slice32(c["rgba"], c["background"], c["grid"]))
    assert np.array_equal(got[..., 3].view(np.uint32), c["rgba"][..., 3].view(np.uint32))


@pytest.mark.parametrize("name", list(br.CASES))
def test_adjoint_bit_for_bit(name):
    """The loss's g' is a given plane; rgba_grad and the grid gradient, every element written, against the restatement."""
    c = br.case(name)
    image, grid = _backward(c, c["out_grad"])
    want_image, want_grid = br.backward32(c["rgba"], c["background"], c["grid"], c["out_grad"])
    assert not np.isnan(grid).any() and _same_bits(grid, want_grid)
    assert _same_bits(image, want_image)
    assert np.abs(want_grid).max() > 0
    # the image gradient alone (a step outside the grids' window): the same bits from one launch
    grids = bilateral.BilateralGrids(1, (1, 1, 1), DEV)
    bg = c["background"] if np.ndim(c["background"]) == 0 else _dev(c["background"])
    alone = torch.full(c["rgba"].shape, NAN, dtype=torch.float32, device=DEV)
    grids.backward_image(_dev(c["grid"]), _dev(c["rgba"]), bg, _dev(c["out_grad"]), rgba_grad=alone)
    torch.cuda.synchronize()
    assert _same_bits(alone, want_image)
    if name == br.NON_FINITE:
        bad, holes = br.non_finite_cotangent(c["out_grad"])
        a, b = _backward(c, bad), _backward(c, holes)
        assert _same_bits(a[1], br.backward32(c["rgba"], c["background"], c["grid"], bad)[1])
        assert _same_bits(a[1], b[1]) and _same_bits(a[0], b[0])                    # the non-finite values count as 0
        zero = _backward(c, np.zeros_like(c["out_grad"]))
        assert not zero[1].view(np.uint32).any()


def test_two_calls_give_the_same_bits():
    c = br.case("shipped")
    a, b = _backward(c, c["out_grad"], 10.0), _backward(c, c["out_grad"], 10.0)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(_slice(c).view(np.uint32), _slice(c).view(np.uint32))


@pytest.mark.parametrize("triple", [(4, 3, 2), (4, 1, 2), (1, 1, 1)])
def test_tv_term_bit_for_bit(triple):
    shape = br.grid_shape(triple)
    rng = np.random.default_rng(11)
    c = dict(rgba=rng.uniform(0.0, 1.0, (19, 21, 4)).astype(F), background=0.0, grid=rng.standard_normal((12,) + shape).astype(F))
    og = (rng.standard_normal((19, 21, 4)) / 400.0).astype(F)
    for cot in (np.zeros_like(og), og):
        got = _backward(c, cot, 2.5)[1]
        assert _same_bits(got, br.backward32(c["rgba"], 0.0, c["grid"], cot, 2.5)[1])
    assert _same_bits(_backward(c, np.zeros_like(og), 2.5)[1], br.tv_term32(c["grid"], 2.5))
    assert _same_bits(_backward(c, og, 0.0)[1], br.backward32(c["rgba"], 0.0, c["grid"], og, 0.0)[1])   # lambda_tv 0 adds nothing


@pytest.mark.parametrize("triple", [(4, 3, 2), (4, 1, 2), (64, 32, 24)])
def test_adam_step_bit_for_bit(triple):
    """Per view: three visits of view 1 against the restatement, view 0 untouched.  (64, 32, 24) has more elements than the step's
    grid of workgroups covers in one stride."""
    g = bilateral.BilateralGrids(2, triple, DEV, lr=0.01)
    rng = np.random.default_rng(3)
    p0 = (g.params[1].cpu().numpy() + rng.uniform(-0.2, 0.2, tuple(g.params[1].shape))).astype(F)
    g.params[1].copy_(_dev(p0))
    want = (p0, np.zeros_like(p0), np.zeros_like(p0), 0)
    for visit in range(3 if triple[0] < 64 else 1):
        grad = (rng.standard_normal(p0.shape) * 10.0 ** rng.uniform(-6, 0, p0.shape)).astype(F)
        grad[..., 0] = 0.0
        g.end(1, _dev(grad))
        want = br.adam32(grad, *want, 0.01, 0.9, 0.999, 1e-15)
        torch.cuda.synchronize()
        assert g.counts.tolist() == [0, visit + 1]
        assert _same_bits(g.params[1], want[0]) and _same_bits(g.m[1], want[1]) and _same_bits(g.v[1], want[2])
    identity = np.zeros(p0.shape, dtype=F)
    identity[0], identity[5], identity[10] = 1.0, 1.0, 1.0
    assert _same_bits(g.params[0], identity) and not g.m[0].any() and not g.v[0].any()


# ---- 2. apply() under autograd ----
def test_apply_under_autograd_against_the_definition():
    """The graph reaches the image and the grid; both gradients and the value within the bound of tests/test_cpu_bilateral.py."""
    c = br.case("edges_plane")
    grids = bilateral.BilateralGrids(1, (5, 4, 3), DEV)
    rgba = _dev(c["rgba"]).requires_grad_(True)
    grid = _dev(c["grid"]).requires_grad_(True)
    out = grids.apply(grid, rgba, _dev(c["background"]))
    assert out.requires_grad and _same_bits(out, br.slice32(c["rgba"], c["background"], c["grid"]))
    (out * _dev(c["out_grad"])).sum().backward()
    torch.cuda.synchronize()
    mag = br.magnitudes(c["rgba"], c["background"], c["grid"], c["out_grad"])
    out64 = br.slice64(c["rgba"], c["background"], c["grid"])
    assert (np.abs(out.detach().cpu().numpy()[..., :3] - out64) <= br.N_SLICE * br.U * mag["out"]).all()
    image64, grid64 = br.backward64(c["rgba"], c["background"], c["grid"], c["out_grad"])
    p = br.pixels32(c["rgba"], c["background"], c["grid"].shape[1:])
    z64, inside64 = br.branches64(c["rgba"], c["background"], c["grid"].shape[1:])
    same = ((z64 == p["z"][:, 0]) & (inside64 == p["inside"])).reshape(image64.shape[:2])
    assert same.mean() >= 0.995
    n_image = np.array([br.N_IMAGE] * 3 + [br.N_ALPHA], dtype=np.float64)
    assert (np.abs(rgba.grad.cpu().numpy() - image64)[same] <= (n_image * br.U * mag["image"])[same]).all()
    bound = br.N_GRID * br.U * mag["grid"] + 0.5 * mag["contributions"] * mag["unit"]
    assert (np.abs(grid.grad.cpu().numpy() - grid64) <= bound).all()
    # without a graph: the same bits, no grad_fn; a view index in the place of the tensor reads the state
    with torch.no_grad():
        assert torch.equal(grids.apply(grid, rgba, _dev(c["background"])), out)
    flat = grids.apply(0, rgba.detach(), 1.0)
    assert not flat.requires_grad and tuple(flat.shape) == tuple(rgba.shape)


# ---- 3. the train step ----
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The reduced synthetic COLMAP scene of tests/test_gpu_environment.py: 16 views of 160 x 160, every 8th held out."""
    root = write_synthetic_colmap(str(tmp_path_factory.mktemp("bilateral") / "scene"), n_views=16, size=160, n_teacher=40_000, n_points=4_000)
    init, tb, vb, extent = load_scene(root)
    return dict(root=root, init=init, tb=tb, vb=vb, extent=extent)


def _smooth_grid(triple, seed, strength=0.15):
    """[12,L,Gh,Gw] float32: the identity plus a smooth part (low-order products of the three coordinates)."""
    L, Gh, Gw = br.grid_shape(triple)
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.linspace(-1, 1, L), np.linspace(-1, 1, Gh), np.linspace(-1, 1, Gw), indexing="ij")
    G = np.zeros((12, L, Gh, Gw))
    G[0], G[5], G[10] = 1.0, 1.0, 1.0
    for k in range(12):
        a = rng.uniform(-strength, strength, 4)
        G[k] += a[0] * x + a[1] * y + a[2] * z + a[3] * x * y * z
    return G.astype(F)


def _one_step(sc, batch, fused_loss, switch=True):
    model = native.NativeGaussianModel(sc["init"], device=DEV, background_color="white")
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=sc["extent"], fused_loss=fused_loss, bilateral_gradient=switch)
    seen, inner = [], st._loss
    st._loss = lambda b, rgba: (seen.append(rgba.clone()), seen.append(inner(b, rgba)), seen[-1])[2]
    loss, out = st.step(batch)
    torch.cuda.synchronize()
    return st, loss, out, seen[1][2], seen[0]


def test_one_step_fused_against_the_torch_branch(scene):
    """A view of the synthetic scene with a mask, over white, a smooth non-identity grid and lambda_tv 10: loss to 1e-5, rgba_grad to
    rel-L2 2e-5 and the grid gradient to rel-L2 1e-4 — the one-step bars of tests/test_gpu_exposure_training.py for the loss, what
    the backward receives (its parameter blocks) and d(loss)/dE.  The fused step IS slice, fused loss over 0 and adjoint of its
    own render, and pred_rgb stays the uncorrected composite."""
    batch = copy.copy(scene["tb"][3])
    H, W = int(batch.rgb_gt.shape[1]), int(batch.rgb_gt.shape[2])
    mask = torch.ones((1, H, W, 1), dtype=torch.float32)
    mask[:, :, :W // 3] = 0.0
    batch.mask = mask.to(DEV)
    G = _dev(_smooth_grid((16, 16, 8), 5))
    batch.bilateral_grid, batch.bilateral_lambda_tv = G, 10.0
    G0 = G.clone()
    fs, floss, fout, fgrad, rgba = _one_step(scene, batch, True)
    ts, tloss, tout, tgrad, trgba = _one_step(scene, batch, False)
    assert torch.equal(rgba, trgba) and torch.equal(G, G0)                         # the same render; the step leaves the caller's grid
    e_image = rel_l2(fgrad.cpu().numpy(), tgrad.cpu().numpy())
    e_grid = rel_l2(fs.bilateral_gradient.cpu().numpy(), ts.bilateral_gradient.cpu().numpy())
    print(f"\n[bilateral step] loss fused {float(floss):.8f} torch {float(tloss):.8f}; rgba_grad rel-L2 {e_image:.3e}; grid gradient rel-L2 {e_grid:.3e}")
    assert abs(float(floss) - float(tloss)) <= 1e-5
    assert e_image <= 2e-5
    assert float(fs.bilateral_gradient.abs().max()) > 0 and e_grid <= 1e-4
    # the fused branch is the three calls on its own render
    grids = bilateral.BilateralGrids(1, (16, 16, 8), DEV)
    sliced = grids.slice(G, rgba, 1.0)
    loss3, out_grad = losses.fused_photometric_loss(sliced, batch.rgb_gt, 0.0, 0.8, 0.2, mask=batch.mask)
    assert float(loss3[0]) == float(floss)
    image, grid_grad = grids.backward(G, rgba, 1.0, out_grad, lambda_tv=10.0)
    assert torch.equal(image, fgrad) and torch.equal(grid_grad, fs.bilateral_gradient)
    assert not bool(fgrad[:, :W // 3].any())                                       # a masked pixel has no gradient
    assert torch.equal(fout["pred_rgb"][0], rgba[..., :3] + (1.0 - rgba[..., 3:]))
    plain3, _ = losses.fused_photometric_loss(rgba, batch.rgb_gt, 1.0, 0.8, 0.2, mask=batch.mask)
    assert abs(float(plain3[0]) - float(floss)) > 1e-3                             # (the grid does change this loss)
    # outside the window: the grid is applied (the same loss, the same image gradient), nothing is left for the optimiser
    off = native.NativeTrainStep(native.NativeGaussianModel(scene["init"], device=DEV, background_color="white"), gut.Tracer({"render": {}}),
                                 scene_extent=scene["extent"], bilateral_gradient=True)
    off.enable_bilateral_gradient(False)
    seen, inner = [], off._loss
    off._loss = lambda b, r: (seen.append(inner(b, r)), seen[-1])[1]
    loss_off, _ = off.step(batch)
    assert float(loss_off) == float(floss) and off.bilateral_gradient is None and torch.equal(seen[0][2], fgrad)
    # a later step without a grid does not keep the previous view's gradient
    plain = copy.copy(scene["tb"][4])
    fs.step(plain)
    assert fs.bilateral_gradient is None
    with pytest.raises(ValueError, match="built without bilateral_gradient=True"):
        native.NativeTrainStep(native.NativeGaussianModel(scene["init"], device=DEV), gut.Tracer({"render": {}})).enable_bilateral_gradient(True)


def test_with_the_switch_and_no_grid_the_step_is_what_it_was():
    """A stepper built with bilateral_gradient=True, given a batch without a grid, against one built without the switch: loss and
    parameters bit for bit.  The backward sums a Gaussian's gradient with float atomics in no fixed order, so the
    inputs fix the order's effect away as tests/test_gpu_trace_refusals.py does: the mask is 1 in two pixels of two different tiles,
    every other pixel's gradient is an exact zero, and every accumulator receives at most two non-zero terms."""
    sc = scenes.scene_c1(4000, 21)
    batch = _batch(False)
    H, W = int(batch.rgb_gt.shape[1]), int(batch.rgb_gt.shape[2])
    mask = torch.zeros((1, H, W, 1), dtype=torch.float32)
    mask[0, 20, 30], mask[0, 45, 70] = 1.0, 1.0
    batch.mask = mask.to(DEV)
    runs = []
    for switch in (True, False, False):
        model = native.NativeGaussianModel(sc, device=DEV)
        st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, bilateral_gradient=switch)
        raw0 = model.raw.clone()
        loss, _ = st.step(batch)
        torch.cuda.synchronize()
        assert not torch.equal(model.raw, raw0) and st.bilateral_gradient is None
        runs.append((float(loss), model.raw.clone(), model.features.clone()))
    with_switch, without, again = runs
    print(f"\n[bilateral off] two steppers without the switch agree: {torch.equal(without[1], again[1]) and torch.equal(without[2], again[2])}")
    assert with_switch[0] == without[0]
    assert torch.equal(with_switch[1], without[1]) and torch.equal(with_switch[2], without[2])


# ---- 4. recovery ----
def _true_grid(view):
    """A known, smooth grid [12,L,Gh,Gw] float64 at the shipped shape: a vignette-like gain falling to about half towards the corners
    times a tone curve over the luminance, with a small colour cast and offset that differ per view."""
    Gw, Gh, L = 16, 16, 8
    z, y, x = np.meshgrid(np.linspace(0, 1, L), np.linspace(-1, 1, Gh), np.linspace(-1, 1, Gw), indexing="ij")
    gain = (1.0 - 0.25 * (x * x + y * y)) * (0.8 + 0.35 * z)                        # 0.5 x tone at the corners
    G = np.zeros((12, L, Gh, Gw))
    cast = (1.0 + 0.05 * view, 1.0, 1.0 - 0.04 * view)
    for i in range(3):
        G[5 * i] = gain * cast[i]
        G[4 * i + 3] = 0.02 * (view - 1) * (1.0 - z)
    return G


def test_known_grids_are_recovered_with_the_gaussians_frozen(scene):
    """Four views of the synthetic scene; each photo is the model's own render pushed through _true_grid(view) by the float64
    definition.  All Gaussian rates are 0; only the grids train: 75 visits per view (300 steps), lr 0.01, lambda_tv 10.  Per view, the
    MSE between the grid-corrected render and the photo ends below the MSE of the best global affine fit of the render to the photo
    (losses.colour_correction: the closed-form optimum of what --exposure can reach).  Measured: see DESIGN.md §21."""
    views = [0, 1, 2, 3]
    model = native.NativeGaussianModel(scene["init"], device=DEV)
    tracer = gut.Tracer({"render": {}})
    batches, comps = [], []
    for v in views:
        b = copy.copy(scene["tb"][v])
        with torch.no_grad():
            comp = tracer.render(model, b, train=False)["pred_rgb"][0].double()
        photo = losses.bilateral_slice(comp, torch.as_tensor(_true_grid(v), device=DEV))
        b.rgb_gt = photo.float()[None].contiguous()
        batches.append(b)
        comps.append(comp)
    grids = bilateral.BilateralGrids(len(views), (16, 16, 8), DEV, lr=0.01)
    st = native.NativeTrainStep(model, tracer, scene_extent=scene["extent"], bilateral_gradient=True)
    st.schedule = None
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    raw0, feat0 = model.raw.clone(), model.features.clone()
    for visit in range(75):
        for v in views:
            st.step(grids.begin(v, batches[v]))
            grids.end(v, st.bilateral_gradient)
    torch.cuda.synchronize()
    assert torch.equal(model.raw, raw0) and torch.equal(model.features, feat0)
    assert grids.counts.tolist() == [75] * len(views)
    ratios = []
    for v in views:
        photo = batches[v].rgb_gt[0].double()
        rgba = torch.cat([comps[v].float(), torch.ones_like(comps[v][..., :1]).float()], dim=-1).contiguous()
        corrected = grids.slice(v, rgba, 0.0)[..., :3].double()
        E = losses.colour_correction(comps[v], photo)
        fitted = losses.apply_exposure(comps[v], E.to(comps[v].device))
        mse_grid, mse_fit = float(((corrected - photo) ** 2).mean()), float(((fitted - photo) ** 2).mean())
        mse_start = float(((comps[v] - photo) ** 2).mean())
        ratios.append(mse_grid / mse_fit)
        print(f"\n[bilateral recovery] view {v}: MSE uncorrected {mse_start:.3e}, best global affine {mse_fit:.3e}, grid {mse_grid:.3e}, "
              f"ratio {ratios[-1]:.4f}")
    assert all(r < 1.0 for r in ratios), ratios


# ---- 5. the trainer ----
NO_EVENTS = dict(densify=dict(start_iteration=-1, end_iteration=-1), prune=dict(start_iteration=-1, end_iteration=-1),
                 reset_density=dict(start_iteration=-1, end_iteration=-1))


def _freeze(tr):
    """All Gaussian rates 0 and no schedule to bring the position rate back: only the grids and the map can move."""
    tr.stepper.schedule = None
    tr.stepper.lr12[:] = 0.0
    tr.stepper.lr48[:] = 0.0
    return tr


def test_trainer_run_with_resume(scene, tmp_path, capsys):
    """`--bilateral` with the environment map on, through the command line: the final JSON has the three keys, bilateral_grids.npy
    and the checkpoint's `native` block hold the grids.  Resume: 28 steps straight against 14 steps, a checkpoint and a Trainer
    resumed from it, with the Gaussians' rates at 0 (the backward's float atomics make a learnt model's bits differ between two
    identical runs, see tests/test_gpu_environment.py): grids, their Adam state and the map are those of the uninterrupted run."""
    root, init, tb, vb, extent = (scene[k] for k in ("root", "init", "tb", "vb", "extent"))
    out_c = str(tmp_path / "cli")
    capsys.readouterr()
    assert trainer_mod.main(["--path", root, "--n-iterations", "6", "--out-dir", out_c, "--environment", "--environment-resolution", "8",
                             "--bilateral", "--bilateral-grid", "8", "6", "4", "--bilateral-lr", "0.005", "--bilateral-tv", "5"]) == 0
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    assert stats["bilateral_grid"] == [8, 6, 4] and stats["bilateral_mean_tv"] > 0 and 0.9 < stats["bilateral_mean_gain"] < 1.1
    assert stats["environment_resolution"] == 8
    saved = np.load(os.path.join(out_c, "bilateral_grids.npy"))
    assert saved.shape == (len(tb), 12, 4, 6, 8) and np.isfinite(saved).all()
    last = torch.load(os.path.join(out_c, "ckpt_last.pt"), map_location="cpu", weights_only=True)["native"]
    assert set(last["bilateral"]) == {"params", "exp_avg", "exp_avg_sq", "counts"} and "environment" in last
    assert np.array_equal(last["bilateral"]["params"].numpy(), saved) and int(last["bilateral"]["counts"].sum()) == 6

    conf = dict(n_iterations=28, val_frequency=10 ** 9, test_last=False, seed=0, environment=dict(enabled=True, resolution=16),
                bilateral=dict(enabled=True, grid=[8, 8, 4], lr=0.01), checkpoint=dict(iterations=[14]),
                strategy=dict(method="GSStrategy", **NO_EVENTS))
    out_f = str(tmp_path / "frozen")
    straight = _freeze(trainer_mod.Trainer(dict(conf, out_dir=out_f), init, tb, test_batches=vb, scene_extent=extent))
    raw0 = straight.model.raw.clone()
    stats = straight.train()
    assert torch.equal(straight.model.raw, raw0)
    assert stats["bilateral_grid"] == [8, 8, 4] and stats["bilateral_mean_tv"] > 0
    mid = os.path.join(out_f, "ours_14", "ckpt_14.pt")
    resumed = _freeze(trainer_mod.Trainer(dict(conf, out_dir="", resume=mid), None, tb, test_batches=vb, scene_extent=extent))
    assert resumed.global_step == 14
    assert torch.equal(resumed.bilateral_grids(), torch.load(mid, map_location="cpu", weights_only=True)["native"]["bilateral"]["params"])
    assert not torch.equal(resumed.bilateral_grids(), straight.bilateral_grids())
    resumed.train()
    assert torch.equal(resumed.bilateral_grids(), straight.bilateral_grids())
    assert torch.equal(resumed.environment(), straight.environment())
    a, b = straight.bilateral.state_dict(), resumed.bilateral.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a) and int(a["counts"].sum()) == 28
    with pytest.raises(ValueError, match="resume with --bilateral"):
        trainer_mod.Trainer(dict(conf, out_dir="", resume=mid, bilateral=dict(enabled=False)), None, tb, scene_extent=extent)
