"""gut_photometric_loss_background and its wrapper against fp64 torch autograd (CPU) of
train.photometric_loss_torch((rgb + B (1 - alpha)) * M, gt * M): every pixel composited over its own background colour B[y,x,:]
(the reference's `random` background, model/background.py:83-89), with and without the mask of trainer.py:397-404.
Tolerances: those of tests/test_gpu_masked_loss.py — |loss diff| <= 5e-6, |L1 diff| <= 2e-6, |SSIM diff| <= 2e-6, gradient rel-L2
<= 1e-4 (fp32 kernels vs an fp64 reference) — plus the exact statements: a masked-out pixel gets 0.0 in all four channels, an
all-zero plane returns what background 0.0 returns, and the constant-background entry points are not rerouted."""
import ctypes as C
import functools
import importlib

import pytest
import torch

from tests.test_gpu_masked_loss import HALF_COLUMN, _mask

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")
capi = importlib.import_module("3dgrut_amd._capi")

LOSS_TOL, L1_TOL, SSIM_TOL, GRAD_TOL = 5e-6, 2e-6, 2e-6, 1e-4
# not multiples of the 16-pixel tile and more than one tile each way; one tile with a single valid SSIM row
SHAPES = [(37, 53), (40, 56), (12, 17)]
MASK_SHAPES = SHAPES[:2]            # _mask's columns (20, 30..40, 45) need a width above 45


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    g = torch.Generator().manual_seed(5)
    return torch.rand((H, W, 4), generator=g), torch.rand((H, W, 3), generator=g), torch.rand((H, W, 3), generator=g)


@functools.lru_cache(maxsize=None)
def _case(H, W, plane="random", masked=False):
    """Inputs (CPU) and the fp64 reference of one (shape, background plane, mask): computed once, shared, not modified."""
    rgba, gt, B = _inputs(H, W)
    if plane == "ones":
        B = torch.ones((H, W, 3))
    mask = _mask(H, W) if masked else torch.ones((H, W))
    r64 = rgba.double().requires_grad_(True)
    m64 = mask.double()[..., None]
    img = (r64[..., :3] + B.double() * (1.0 - r64[..., 3:])) * m64
    gtm = gt.double() * m64
    ref = train.photometric_loss_torch(img.unsqueeze(0), gtm.unsqueeze(0), window=train._gauss_window(dtype=torch.float64))
    ref.backward()
    loss, l1 = float(ref.detach()), float((img - gtm).detach().abs().mean())
    # (the reference's SSIM from its own loss = 0.8 L1 + 0.2 (1 - SSIM), all in fp64)
    return dict(rgba=rgba, gt=gt, B=B, mask=mask if masked else None, loss=loss, l1=l1, ssim=1.0 - (loss - 0.8 * l1) / 0.2,
                grad=r64.grad.detach())


def _call(H, W, rgba, gt, B, mask=None):
    """One raw call of gut_photometric_loss_background (mask a device tensor or None = NULL) into NaN-filled outputs."""
    lib = capi.load()
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gut_photometric_loss_background(st, H, W, rgba.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(),
                                             B.data_ptr(), 0.8, 0.2, ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad


def _constant(H, W, rgba, gt, bg):
    """gut_photometric_loss with a constant background, into NaN-filled outputs."""
    lib = capi.load()
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.gut_photometric_loss(C.c_void_p(torch.cuda.current_stream().cuda_stream), H, W, rgba.data_ptr(), gt.data_ptr(), bg, 0.8, 0.2,
                                  ws.data_ptr(), out3.data_ptr(), grad.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad


def _run(c, H, W):
    x, y, b = c["rgba"].cuda().contiguous(), c["gt"].cuda().contiguous(), c["B"].cuda().contiguous()
    m = None if c["mask"] is None else c["mask"].cuda().contiguous()
    return _call(H, W, x, y, b, m)


def _check(tag, c, out3, grad):
    """The tolerances of the module docstring; returns the gradient as fp64 on the CPU."""
    o = out3.cpu().double()
    got = grad.cpu().double()
    err = float((got - c["grad"]).norm() / c["grad"].norm())
    print(f"\n[background loss {tag}] loss {float(o[0]):.8f} ref {c['loss']:.8f}, L1 {float(o[1]):.8f} ref {c['l1']:.8f}, "
          f"SSIM {float(o[2]):.8f} ref {c['ssim']:.8f}, gradient rel-L2 {err:.3e}")
    assert torch.isfinite(o).all() and torch.isfinite(got).all()          # every output element was written
    assert abs(float(o[0]) - c["loss"]) <= LOSS_TOL
    assert abs(float(o[1]) - c["l1"]) <= L1_TOL
    assert abs(float(o[2]) - c["ssim"]) <= SSIM_TOL
    assert err <= GRAD_TOL, err
    return got


@pytest.mark.parametrize("hw", SHAPES)
def test_loss_and_gradient_match_the_reference(hw):
    H, W = hw
    c = _case(H, W)
    _check(f"{H}x{W}", c, *_run(c, H, W))


@pytest.mark.parametrize("hw", SHAPES)
def test_alpha_gradient_alone(hw):
    """-(B_r g_r + B_g g_g + B_b g_b) per pixel: a constant-background alpha pass would pass the whole-tensor check (the alpha
    channel is a small part of the norm) and fail here."""
    H, W = hw
    c = _case(H, W)
    _, grad = _run(c, H, W)
    ref = c["grad"][..., 3]
    assert float(ref.norm()) > 0
    err = float((grad.cpu().double()[..., 3] - ref).norm() / ref.norm())
    print(f"\n[background loss {H}x{W}] alpha gradient rel-L2 {err:.3e}")
    assert err <= GRAD_TOL, err


@pytest.mark.parametrize("hw", MASK_SHAPES)
def test_with_a_mask(hw):
    H, W = hw
    c = _case(H, W, masked=True)
    out3, grad = _run(c, H, W)
    got = _check(f"{H}x{W} masked", c, out3, grad)
    ref_a = c["grad"][..., 3]
    assert float((got[..., 3] - ref_a).norm() / ref_a.norm()) <= GRAD_TOL
    off = c["mask"] == 0
    assert int(off.sum()) > 0 and bool((c["grad"][off] == 0).all())     # (the reference's own gradient is exactly zero there)
    assert bool((grad.cpu()[off] == 0.0).all())                         # all four channels, exactly
    assert float(got[:, HALF_COLUMN, :3].abs().max()) > 0 and float(got[:, HALF_COLUMN, 3].abs().max()) > 0   # the 0.5 column


@pytest.mark.parametrize("hw", SHAPES)
def test_zero_plane_equals_the_black_constant_form(hw):
    H, W = hw
    rgba, gt, _ = _inputs(H, W)
    x, y = rgba.cuda().contiguous(), gt.cuda().contiguous()
    z3, zg = _call(H, W, x, y, torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"))
    k3, kg = _constant(H, W, x, y, 0.0)
    assert torch.isfinite(k3).all() and torch.isfinite(kg).all()
    assert torch.equal(z3, k3) and torch.equal(zg, kg)


@pytest.mark.parametrize("hw", SHAPES)
def test_ones_plane_matches_the_white_reference(hw):
    """(Bit equality with the constant form is not asked for: -(g_r + g_g + g_b) is rounded in another order.)"""
    H, W = hw
    c = _case(H, W, "ones")
    got = _check(f"{H}x{W} ones", c, *_run(c, H, W))
    ref_a = c["grad"][..., 3]
    assert float((got[..., 3] - ref_a).norm() / ref_a.norm()) <= GRAD_TOL


@pytest.mark.parametrize("background", ["black", "white"])
@pytest.mark.parametrize("hw", SHAPES[:2])
def test_constant_backgrounds_are_not_rerouted(background, hw):
    H, W = hw
    rgba, gt, _ = _inputs(H, W)
    x, y = rgba.cuda().contiguous(), gt.cuda().contiguous()
    bits = lambda t: t.view(torch.int32)
    k3, kg = _constant(H, W, x, y, 1.0 if background == "white" else 0.0)
    w3, wg = losses.fused_photometric_loss(x, y, background, 0.8, 0.2)
    assert torch.equal(bits(w3), bits(k3)) and torch.equal(bits(wg), bits(kg))
    m = _mask(H, W).cuda()
    lib = capi.load()
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    m3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    mg = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.gut_photometric_loss_masked(C.c_void_p(torch.cuda.current_stream().cuda_stream), H, W, x.data_ptr(), y.data_ptr(), m.data_ptr(),
                                         1.0 if background == "white" else 0.0, 0.8, 0.2, ws.data_ptr(), m3.data_ptr(), mg.data_ptr())
    assert rc == 0
    w3, wg = losses.fused_photometric_loss(x, y, background, 0.8, 0.2, mask=m)
    assert torch.equal(bits(w3), bits(m3)) and torch.equal(bits(wg), bits(mg))


def test_wrapper_background_forms():
    H, W = SHAPES[1]
    rgba, gt, B = _inputs(H, W)
    x, y, b = rgba.cuda().contiguous(), gt.cuda().contiguous(), B.cuda().contiguous()
    bits = lambda t: t.view(torch.int32)
    raw3, rawg = _call(H, W, x, y, b)
    for form in (b, b[None], B, b.double(), B.double()[None]):
        o3, og = losses.fused_photometric_loss(x, y, form, 0.8, 0.2)
        assert torch.equal(bits(o3), bits(raw3)) and torch.equal(bits(og), bits(rawg)), (tuple(form.shape), form.dtype, form.device)
    m = _mask(H, W).cuda()
    o3, og = losses.fused_photometric_loss(x[None], y[None], b, 0.8, 0.2, mask=m[None, :, :, None])
    r3, rg = _call(H, W, x, y, b, m)
    assert torch.equal(bits(o3), bits(r3)) and torch.equal(bits(og), bits(rg))
    colour = torch.tensor([0.25, 0.5, 0.875])
    e3, eg = _call(H, W, x, y, colour.cuda().expand(H, W, 3).contiguous())
    for form in (colour, colour.cuda(), colour.double()):
        o3, og = losses.fused_photometric_loss(x, y, form, 0.8, 0.2)
        assert torch.equal(bits(o3), bits(e3)) and torch.equal(bits(og), bits(eg))
    for bad in (b[..., 0], torch.cat([b, b[..., :1]], -1), b[None].expand(2, H, W, 3), b.transpose(0, 1)):
        with pytest.raises(ValueError, match="background"):
            losses.fused_photometric_loss(x, y, bad, 0.8, 0.2)


def test_null_background_and_small_images_are_refused():
    lib = capi.load()
    H, W = SHAPES[0]
    t = torch.zeros((H * W * 4,), dtype=torch.float32, device="cuda")
    ws = torch.empty(((lib.gut_photometric_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = t.data_ptr()
    assert lib.gut_photometric_loss_background(st, H, W, p, p, None, None, 0.8, 0.2, ws.data_ptr(), p, p) == 1
    assert lib.gut_photometric_loss_background(st, H, W, p, None, None, p, 0.8, 0.2, ws.data_ptr(), p, p) == 1
    assert lib.gut_photometric_loss_background(st, 10, W, p, p, None, p, 0.8, 0.2, ws.data_ptr(), p, p) == 1
    assert lib.gut_photometric_loss_background(st, H, 10, p, p, None, p, 0.8, 0.2, ws.data_ptr(), p, p) == 1
