"""gut_photometric_loss_exposure, its wrapper and gut_exposure_adam_step.

Yardstick: fp64 torch autograd on the CPU of losses.photometric_loss(rgb + B (1 - alpha), gt, mask=M, exposure=E), the torch
definition of the affine image — never the code under test.  Tolerances are those of tests/test_gpu_masked_loss.py and
tests/test_gpu_background_loss.py, which run the same fp32 kernels against fp64: |loss| <= 5e-6, |L1| <= 2e-6, |SSIM| <= 2e-6,
d rgba rel-L2 <= 1e-4, the alpha channel alone rel-L2 <= 1e-4, and dE (12 values) rel-L2 <= 1e-4.  For these inputs no entry of the
fp64 dE cancels (evaluated on the CPU: the smallest entry is 0.32 - 0.67 of the largest over a white background or a plane, 0.17 -
0.19 over black, 0.045 over black at 12 x 17; asserted below at 0.03 on the reference alone) and fp32 and fp64 torch evaluations
differ by 3e-7 rel-L2 or less, so the bounds leave room for the kernels' own summation order and nothing else.  Plus the exact
statements: identical calls give identical bits, a masked-out pixel gets 0.0 four times and adds nothing, a NULL gradient output
changes no other bit, and the entry points without an exposure are not rerouted."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from tests.test_gpu_masked_loss import _mask

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
exposure = importlib.import_module("3dgrut_amd.exposure")
capi = importlib.import_module("3dgrut_amd._capi")

LOSS_TOL, L1_TOL, SSIM_TOL, GRAD_TOL = 5e-6, 2e-6, 2e-6, 1e-4
# partial tiles both ways, more than one tile; a single tile with one valid SSIM row
SHAPES = [(37, 53), (40, 56), (12, 17)]
MASK_SHAPES = SHAPES[:2]            # _mask's columns (20, 30..40, 45) need a width above 45
E_TEST = torch.tensor([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.03], [0.02, -0.05, 1.20, 0.04]], dtype=torch.float32)
IDENTITY = torch.tensor(exposure.IDENTITY, dtype=torch.float32)
# (background, masked): constant black, constant white, plane, plane + mask, white + mask
COMBOS = [("black", False), ("white", False), ("plane", False), ("plane", True), ("white", True)]
CASES = [(hw, bg, m) for bg, m in COMBOS for hw in (MASK_SHAPES if m else SHAPES)]
bits = lambda t: t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    g = torch.Generator().manual_seed(5)
    return torch.rand((H, W, 4), generator=g), torch.rand((H, W, 3), generator=g), torch.rand((H, W, 3), generator=g)


@functools.lru_cache(maxsize=None)
def _case(H, W, background, masked):
    """Inputs (CPU) and the fp64 reference of one (shape, background, mask): computed once, shared, not modified."""
    rgba, gt, B = _inputs(H, W)
    mask = _mask(H, W) if masked else None
    bg64 = B.double() if background == "plane" else (1.0 if background == "white" else 0.0)
    r64 = rgba.double().requires_grad_(True)
    E64 = E_TEST.double().requires_grad_(True)
    comp = r64[..., :3] + bg64 * (1.0 - r64[..., 3:])
    m4 = None if mask is None else mask.double()[None, :, :, None]
    ref = losses.photometric_loss(comp[None], gt.double()[None], 0.8, 0.2, mask=m4, exposure=E64)
    ref.backward()
    with torch.no_grad():
        img = losses.apply_exposure(comp, E64)
        gtm = gt.double()
        if mask is not None:
            img, gtm = img * mask.double()[..., None], gtm * mask.double()[..., None]
        l1 = float((img - gtm).abs().mean())
    loss = float(ref.detach())
    return dict(rgba=rgba, gt=gt, B=B if background == "plane" else None, bg=1.0 if background == "white" else 0.0, mask=mask, loss=loss,
                l1=l1, ssim=1.0 - (loss - 0.8 * l1) / 0.2, grad=r64.grad.detach(), dE=E64.grad.detach().reshape(12))


def _call(H, W, rgba, gt, E, bg=0.0, B=None, mask=None, want_dE=True, ws=None):
    """One raw call of gut_photometric_loss_exposure (device tensors; B / mask None = NULL) into NaN-filled outputs."""
    lib = capi.load()
    if ws is None:
        ws = torch.empty(((lib.gut_photometric_exposure_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    dE = torch.full((12,), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gut_photometric_loss_exposure(st, H, W, rgba.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(),
                                           None if B is None else B.data_ptr(), bg, E.data_ptr(), 0.8, 0.2, ws.data_ptr(), out3.data_ptr(),
                                           grad.data_ptr(), dE.data_ptr() if want_dE else None)
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad, dE


def _dev(c, E=E_TEST):
    d = lambda t: None if t is None else t.cuda().contiguous()
    return dict(rgba=d(c["rgba"]), gt=d(c["gt"]), E=E.reshape(12).cuda().contiguous(), bg=c["bg"], B=d(c["B"]), mask=d(c["mask"]))


@pytest.mark.parametrize("hw,background,masked", CASES)
def test_loss_gradients_and_exposure_gradient_match_the_reference(hw, background, masked):
    H, W = hw
    c = _case(H, W, background, masked)
    out3, grad, dE = _call(H, W, **_dev(c))
    o, got, gotE = out3.cpu().double(), grad.cpu().double(), dE.cpu().double()
    err = float((got - c["grad"]).norm() / c["grad"].norm())
    ref_a = c["grad"][..., 3]
    err_a = float((got[..., 3] - ref_a).norm() / ref_a.norm()) if float(ref_a.norm()) > 0 else float(got[..., 3].abs().max())
    err_E = float((gotE - c["dE"]).norm() / c["dE"].norm())
    spread = float(c["dE"].abs().min() / c["dE"].abs().max())
    print(f"\n[exposure loss {H}x{W} {background} masked={masked}] loss {float(o[0]):.8f} ref {c['loss']:.8f}, L1 {float(o[1]):.8f} ref "
          f"{c['l1']:.8f}, SSIM {float(o[2]):.8f} ref {c['ssim']:.8f}, d rgba rel-L2 {err:.3e}, alpha {err_a:.3e}, dE {err_E:.3e} "
          f"(smallest |dE| / largest {spread:.2f})")
    assert torch.isfinite(o).all() and torch.isfinite(got).all() and torch.isfinite(gotE).all()   # every output element was written
    assert spread >= 0.03                                    # no entry of the reference is a cancellation
    assert abs(float(o[0]) - c["loss"]) <= LOSS_TOL
    assert abs(float(o[1]) - c["l1"]) <= L1_TOL
    assert abs(float(o[2]) - c["ssim"]) <= SSIM_TOL
    assert err <= GRAD_TOL, err
    if background == "black":
        assert float(ref_a.abs().max()) == 0.0 and err_a == 0.0     # constant black: the alpha gradient is exactly zero
    else:
        assert float(ref_a.norm()) > 0 and err_a <= GRAD_TOL, err_a
    assert err_E <= GRAD_TOL, err_E
    if masked:
        off = c["mask"] == 0
        assert int(off.sum()) > 0 and bool((c["grad"][off] == 0).all())     # (the reference's own gradient is exactly zero there)
        assert bool((grad.cpu()[off] == 0.0).all())                         # all four channels, exactly


@pytest.mark.parametrize("hw,background,masked", [(SHAPES[0], "plane", True), (SHAPES[1], "white", False), (SHAPES[2], "black", False)])
def test_identical_calls_give_identical_bits(hw, background, masked):
    H, W = hw
    d = _dev(_case(H, W, background, masked))
    a, b = _call(H, W, **d), _call(H, W, **d)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


@pytest.mark.parametrize("hw,background", [(MASK_SHAPES[0], "plane"), (MASK_SHAPES[1], "white")])
def test_masked_out_pixels_add_exactly_nothing(hw, background):
    """Other (finite) values in rgba, gt and the background AT masked-out pixels: loss3, dE and every other pixel's gradient keep
    their bits, and the masked-out pixels keep their four zeros."""
    H, W = hw
    c = _case(H, W, background, True)
    d = _dev(c)
    base3, baseg, baseE = _call(H, W, **d)
    off = (c["mask"] == 0).cuda()
    g = torch.Generator().manual_seed(9)
    other = dict(d)
    other["rgba"] = torch.where(off[..., None], (torch.rand((H, W, 4), generator=g) * 7.0 - 3.0).cuda(), d["rgba"]).contiguous()
    other["gt"] = torch.where(off[..., None], (torch.rand((H, W, 3), generator=g) * 5.0 - 2.0).cuda(), d["gt"]).contiguous()
    if d["B"] is not None:
        other["B"] = torch.where(off[..., None], (torch.rand((H, W, 3), generator=g) * 9.0 - 4.0).cuda(), d["B"]).contiguous()
    assert not torch.equal(other["rgba"], d["rgba"]) and not torch.equal(other["gt"], d["gt"])
    o3, og, oE = _call(H, W, **other)
    assert torch.equal(bits(o3), bits(base3)) and torch.equal(bits(oE), bits(baseE)) and torch.equal(bits(og), bits(baseg))
    assert bool((og[off] == 0.0).all()) and bool((og[~off][:, :3] != 0.0).any())


@pytest.mark.parametrize("hw,background,masked", [(SHAPES[0], "plane", True), (SHAPES[0], "black", False), (SHAPES[1], "white", False)])
def test_null_gradient_output_applies_the_exposure_and_reduces_nothing(hw, background, masked):
    H, W = hw
    d = _dev(_case(H, W, background, masked))
    lib = capi.load()
    ws = torch.full(((lib.gut_photometric_exposure_workspace_bytes(H, W) + 3) // 4,), 7.0, dtype=torch.float32, device="cuda")
    base_words = (lib.gut_photometric_workspace_bytes(H, W) + 3) // 4
    n3, ng, sentinel = _call(H, W, **d, want_dE=False, ws=ws)
    assert bool(torch.isnan(sentinel).all())                    # the 12 floats that WOULD have been the output: untouched
    assert bool((ws[base_words:] == 7.0).all())                 # no partial was written either
    w3, wg, wE = _call(H, W, **d, ws=ws)
    assert torch.isfinite(wE).all() and not bool((ws[base_words:base_words + 12] == 7.0).all())
    assert torch.equal(bits(n3), bits(w3)) and torch.equal(bits(ng), bits(wg))
    assert torch.isfinite(ng).all()


def test_nulls_and_small_images_are_refused():
    lib = capi.load()
    H, W = SHAPES[0]
    t = torch.zeros((H * W * 4,), dtype=torch.float32, device="cuda")
    ws = torch.empty(((lib.gut_photometric_exposure_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, w = t.data_ptr(), ws.data_ptr()
    f = lib.gut_photometric_loss_exposure
    assert f(st, H, W, None, p, None, None, 0.0, p, 0.8, 0.2, w, p, p, p) == 1     # rgba
    assert f(st, H, W, p, None, None, None, 0.0, p, 0.8, 0.2, w, p, p, p) == 1     # ground truth
    assert f(st, H, W, p, p, None, None, 0.0, None, 0.8, 0.2, w, p, p, p) == 1     # the exposure itself
    assert f(st, H, W, p, p, None, None, 0.0, p, 0.8, 0.2, None, p, p, p) == 1     # workspace
    assert f(st, H, W, p, p, None, None, 0.0, p, 0.8, 0.2, w, None, p, p) == 1     # loss3
    assert f(st, H, W, p, p, None, None, 0.0, p, 0.8, 0.2, w, p, None, p) == 1     # rgba_grad
    assert f(st, 10, W, p, p, None, None, 0.0, p, 0.8, 0.2, w, p, p, p) == 1
    assert f(st, H, 10, p, p, None, None, 0.0, p, 0.8, 0.2, w, p, p, None) == 1
    a = lib.gut_exposure_adam_step
    assert a(st, None, p, p, p, p, 1e-3, 0.9, 0.999, 1e-15) == 1 and a(st, p, None, p, p, p, 1e-3, 0.9, 0.999, 1e-15) == 1
    assert a(st, p, p, None, p, p, 1e-3, 0.9, 0.999, 1e-15) == 1 and a(st, p, p, p, None, p, 1e-3, 0.9, 0.999, 1e-15) == 1
    assert a(st, p, p, p, p, None, 1e-3, 0.9, 0.999, 1e-15) == 1
    torch.cuda.synchronize()
    assert not t.any()                                           # nothing was launched


def _existing(H, W, d):
    """The matching entry point without an exposure, into NaN-filled outputs."""
    lib = capi.load()
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, y, m = d["rgba"].data_ptr(), d["gt"].data_ptr(), None if d["mask"] is None else d["mask"].data_ptr()
    if d["B"] is not None:
        rc = lib.gut_photometric_loss_background(st, H, W, x, y, m, d["B"].data_ptr(), 0.8, 0.2, ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    elif m is not None:
        rc = lib.gut_photometric_loss_masked(st, H, W, x, y, m, d["bg"], 0.8, 0.2, ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    else:
        rc = lib.gut_photometric_loss(st, H, W, x, y, d["bg"], 0.8, 0.2, ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad


@pytest.mark.parametrize("hw,background,masked", CASES)
def test_identity_exposure_agrees_with_the_form_without_one(hw, background, masked):
    """(Bit equality is not asked for: A^T g and the fma chain of the affine image round differently.)"""
    H, W = hw
    d = _dev(_case(H, W, background, masked), E=IDENTITY)
    e3, eg, eE = _call(H, W, **d)
    k3, kg = _existing(H, W, d)
    diff = (e3 - k3).abs().cpu().tolist()
    err = float((eg.double() - kg.double()).norm() / kg.double().norm())
    print(f"\n[identity exposure {H}x{W} {background} masked={masked}] loss3 differences {diff}, d rgba rel-L2 {err:.3e}")
    assert torch.isfinite(eg).all() and torch.isfinite(eE).all()
    assert diff[0] <= LOSS_TOL and diff[1] <= L1_TOL and diff[2] <= SSIM_TOL and err <= GRAD_TOL


@pytest.mark.parametrize("background,masked", [("black", False), ("white", False), ("white", True), ("plane", False)])
def test_forms_without_an_exposure_are_not_rerouted(background, masked):
    H, W = SHAPES[0]
    d = _dev(_case(H, W, background, masked))
    k3, kg = _existing(H, W, d)
    out = losses.fused_photometric_loss(d["rgba"], d["gt"], d["B"] if d["B"] is not None else background, 0.8, 0.2, mask=d["mask"])
    assert len(out) == 2
    assert torch.equal(bits(out[0]), bits(k3)) and torch.equal(bits(out[1]), bits(kg))


def test_exposure_adam_kernel_equals_the_host_arithmetic():
    """gut_exposure_adam_step against ExposureCompensation's host-tensor form over three visits of one view out of two: the same
    fp32 operations (rtol 1e-6 on the moments, 1e-5 on the parameters: the bounds of the pose Adam test); the other view's rows
    keep their bits."""
    cpu = exposure.ExposureCompensation(2, "cpu", lr=1e-3)
    dev = exposure.ExposureCompensation(2, "cuda:0", lr=1e-3)
    rng = np.random.default_rng(2)
    for visit in range(3):
        g = torch.as_tensor(rng.standard_normal(12) * 10.0 ** rng.integers(-3, 3), dtype=torch.float32)
        cpu.end(1, g)
        dev.end(1, g.cuda())
        torch.cuda.synchronize()
        assert dev.counts.tolist() == [0, visit + 1] == cpu.counts.tolist()
        assert torch.allclose(dev.m.cpu(), cpu.m, rtol=1e-6, atol=0) and torch.allclose(dev.v.cpu(), cpu.v, rtol=1e-6, atol=0)
        assert torch.allclose(dev.params.cpu(), cpu.params, rtol=1e-5, atol=0)
        # ... and the CHANGE of the parameters, which rtol on values near 1 hardly sees
        assert torch.allclose(dev.params.cpu()[1] - IDENTITY, cpu.params[1] - IDENTITY, rtol=1e-3, atol=1e-9)
        assert torch.equal(dev.params[0].cpu(), IDENTITY) and not dev.m[0].any() and not dev.v[0].any()
    assert float((dev.params[1].cpu() - IDENTITY).abs().min()) > 1e-4      # every entry moved, by about a rate per visit


def test_wrapper_forms():
    H, W = SHAPES[1]
    d = _dev(_case(H, W, "plane", True))
    raw3, rawg, rawE = _call(H, W, **d)
    x, y, b, m = d["rgba"], d["gt"], d["B"], d["mask"]
    for E in (d["E"], d["E"].reshape(3, 4)):
        for lead in (False, True):
            out = losses.fused_photometric_loss(x[None] if lead else x, y[None] if lead else y, b, 0.8, 0.2, mask=m, exposure=E)
            assert len(out) == 3 and tuple(out[2].shape) == (12,)
            assert torch.equal(bits(out[0]), bits(raw3)) and torch.equal(bits(out[1]), bits(rawg)) and torch.equal(bits(out[2]), bits(rawE))
    out = losses.fused_photometric_loss(x, y, b, 0.8, 0.2, mask=m, exposure=d["E"], exposure_grad=False)
    assert len(out) == 3 and out[2] is None and torch.equal(bits(out[0]), bits(raw3)) and torch.equal(bits(out[1]), bits(rawg))
    row = torch.stack([IDENTITY, E_TEST.reshape(12)]).cuda()[1]             # a row of a [V,12] state: consumed in place
    out = losses.fused_photometric_loss(x, y, b, 0.8, 0.2, mask=m, exposure=row)
    assert torch.equal(bits(out[2]), bits(rawE))
    w3, wg, wE = losses.fused_photometric_loss(x, y, "white", 0.8, 0.2, exposure=d["E"])
    k3, kg, kE = _call(H, W, x, y, d["E"], bg=1.0)
    assert torch.equal(bits(w3), bits(k3)) and torch.equal(bits(wg), bits(kg)) and torch.equal(bits(wE), bits(kE))
    for bad in (d["E"][:11], d["E"].reshape(4, 3), d["E"].reshape(1, 12), d["E"].double(), d["E"].cpu(), [1.0] * 12):
        with pytest.raises(ValueError, match="exposure"):
            losses.fused_photometric_loss(x, y, b, 0.8, 0.2, exposure=bad)
    small = torch.empty((16,), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        losses.fused_photometric_loss(x, y, b, 0.8, 0.2, exposure=d["E"], workspace=small)
