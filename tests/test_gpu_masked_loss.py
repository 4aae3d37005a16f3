"""gut_photometric_loss_masked and its wrappers against fp64 torch autograd (CPU) of
train.photometric_loss_torch((rgb + background (1 - alpha)) * M, gt * M), the reference's masked loss (trainer.py:397-404).
Tolerances: those of tests/test_gpu_losses.py — |loss diff| <= 5e-6, |L1 diff| <= 2e-6, gradient rel-L2 <= 1e-4 (fp32 kernels vs an fp64
reference) — plus two exact statements: a pixel whose mask is 0 gets 0.0 in all four channels, and without a mask (or with an
all-ones one) the entry point returns the bits of gut_photometric_loss."""
import ctypes as C
import functools
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")
capi = importlib.import_module("3dgrut_amd._capi")

LOSS_TOL, L1_TOL, SSIM_TOL, GRAD_TOL = 5e-6, 2e-6, 2e-6, 1e-4
SHAPES = [(37, 53), (40, 56)]      # not multiples of the 16-pixel tile, more than one tile each way
HALF_COLUMN = 45


def _mask(H, W):
    """Columns < 20 zero (an edge inside a tile and inside its neighbours' halo), rows 10..13 x columns 30..40 zero (a hole across
    the x = 32 tile border), one column at 0.5 (values multiply through as they are)."""
    m = torch.ones((H, W), dtype=torch.float32)
    m[:, :20] = 0.0
    m[10:14, 30:41] = 0.0
    m[:, HALF_COLUMN] = 0.5
    return m


@functools.lru_cache(maxsize=None)
def _case(H, W, background):
    """Inputs (CPU) and the fp64 reference of one (shape, background): computed once, shared, not modified."""
    g = torch.Generator().manual_seed(3)
    rgba = torch.rand((H, W, 4), generator=g)
    gt = torch.rand((H, W, 3), generator=g)
    mask = _mask(H, W)
    bg = 1.0 if background == "white" else 0.0
    r64 = rgba.double().requires_grad_(True)
    m64 = mask.double()[..., None]
    img = (r64[..., :3] + bg * (1.0 - r64[..., 3:])) * m64
    gtm = gt.double() * m64
    ref = train.photometric_loss_torch(img.unsqueeze(0), gtm.unsqueeze(0), window=train._gauss_window(dtype=torch.float64))
    ref.backward()
    return dict(rgba=rgba, gt=gt, mask=mask, bg=bg, loss=float(ref.detach()), l1=float((img - gtm).detach().abs().mean()), grad=r64.grad.detach())


def _call(entry, H, W, rgba, gt, bg, mask="absent"):
    """One raw call of gut_photometric_loss (mask "absent") or gut_photometric_loss_masked (mask a device tensor or None = NULL)
    into NaN-filled outputs."""
    lib = capi.load()
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "plain":
        rc = lib.gut_photometric_loss(st, H, W, rgba.data_ptr(), gt.data_ptr(), bg, 0.8, 0.2, ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    else:
        rc = lib.gut_photometric_loss_masked(st, H, W, rgba.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), bg, 0.8, 0.2,
                                             ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad


@pytest.mark.parametrize("background", ["black", "white"])
@pytest.mark.parametrize("hw", SHAPES)
def test_masked_loss_and_gradient_match_the_reference(background, hw):
    H, W = hw
    c = _case(H, W, background)
    x, y, m = c["rgba"].cuda().contiguous(), c["gt"].cuda().contiguous(), c["mask"].cuda().contiguous()
    out3, grad = _call("masked", H, W, x, y, c["bg"], m)
    o = out3.cpu().double()
    got = grad.cpu().double()
    err = float((got - c["grad"]).norm() / c["grad"].norm())
    print(f"\n[masked loss {H}x{W} {background}] loss {float(o[0]):.8f} ref {c['loss']:.8f}, L1 {float(o[1]):.8f} ref {c['l1']:.8f}, "
          f"gradient rel-L2 {err:.3e}")
    assert abs(float(o[0]) - c["loss"]) <= LOSS_TOL
    assert abs(float(o[1]) - c["l1"]) <= L1_TOL
    assert torch.isfinite(got).all()
    assert err <= GRAD_TOL, err
    off = c["mask"] == 0
    assert int(off.sum()) > 0 and bool((c["grad"][off] == 0).all())     # (the reference's own gradient is exactly zero there)
    assert bool((grad.cpu()[off] == 0.0).all())                         # all four channels, exactly
    half = got[:, HALF_COLUMN, :3]
    assert float(half.abs().max()) > 0                                  # the 0.5 column does take a gradient


@pytest.mark.parametrize("background", ["black", "white"])
@pytest.mark.parametrize("hw", SHAPES)
def test_without_a_mask_the_bits_are_those_of_the_unmasked_entry_point(background, hw):
    H, W = hw
    c = _case(H, W, background)
    x, y = c["rgba"].cuda().contiguous(), c["gt"].cuda().contiguous()
    ref3, refg = _call("plain", H, W, x, y, c["bg"])
    assert torch.isfinite(ref3).all() and torch.isfinite(refg).all()
    bits = lambda t: t.view(torch.int32)
    null3, nullg = _call("masked", H, W, x, y, c["bg"], None)            # NULL: the unmasked instantiations
    assert torch.equal(bits(null3), bits(ref3)) and torch.equal(bits(nullg), bits(refg))
    ones = torch.ones((H, W), dtype=torch.float32, device="cuda")        # the masked instantiations; a product with 1.0f is exact
    one3, oneg = _call("masked", H, W, x, y, c["bg"], ones)
    assert torch.equal(bits(one3), bits(ref3)) and torch.equal(bits(oneg), bits(refg))
    # the wrapper routes None to the unmasked entry point too
    w3, wg = losses.fused_photometric_loss(x, y, background, 0.8, 0.2)
    assert torch.equal(bits(w3), bits(ref3)) and torch.equal(bits(wg), bits(refg))


@pytest.mark.parametrize("background", ["black", "white"])
def test_all_zero_mask(background):
    H, W = SHAPES[0]
    c = _case(H, W, background)
    x, y = c["rgba"].cuda().contiguous(), c["gt"].cuda().contiguous()
    out3, grad = _call("masked", H, W, x, y, c["bg"], torch.zeros((H, W), dtype=torch.float32, device="cuda"))
    o = out3.cpu().double()
    assert abs(float(o[0])) <= LOSS_TOL and abs(float(o[1])) <= L1_TOL and abs(float(o[2]) - 1.0) <= SSIM_TOL
    assert bool((grad == 0.0).all())


def test_wrapper_mask_shapes_and_the_autograd_form():
    H, W = SHAPES[1]
    c = _case(H, W, "black")
    x, y = c["rgba"].cuda().contiguous(), c["gt"].cuda().contiguous()
    binary = (c["mask"] == 1.0)                                         # a bool mask: the 0.5 column reads as 0
    m = binary.float().cuda()
    base3, baseg = losses.fused_photometric_loss(x, y, "black", 0.8, 0.2, mask=m)
    raw3, rawg = _call("masked", H, W, x, y, 0.0, m)
    assert torch.equal(base3, raw3) and torch.equal(baseg, rawg)
    for form in (m[..., None], m[None, :, :, None], binary.cuda(), binary, m.double(), m[None, :, :, None].expand(1, H, W, 1)):
        o3, og = losses.fused_photometric_loss(x[None], y[None], 0.0, 0.8, 0.2, mask=form)
        assert torch.equal(o3, base3) and torch.equal(og, baseg), (tuple(form.shape), form.dtype)
    for bad in (m[:, :-1], m[:-1], m[None], m[None, :, :, None].expand(2, H, W, 1), m.t()):
        with pytest.raises(ValueError, match="mask"):
            losses.fused_photometric_loss(x, y, "black", 0.8, 0.2, mask=bad)
    # the autograd form: both images times the mask, then the unmasked HIP SSIM + torch L1
    pred = c["rgba"][None, :, :, :3].cuda().contiguous().requires_grad_(True)
    mask4 = c["mask"][None, :, :, None].cuda()
    loss = losses.photometric_loss(pred, y[None], 0.8, 0.2, mask=mask4)
    assert abs(float(loss.detach()) - c["loss"]) <= LOSS_TOL
    loss.backward()
    got = pred.grad[0].cpu().double()
    ref = c["grad"][..., :3]
    assert float((got - ref).norm() / ref.norm()) <= GRAD_TOL
    assert bool((got[c["mask"] == 0] == 0.0).all())
