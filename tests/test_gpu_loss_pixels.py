"""The loss kernels of csrc/gut_ssim.hip per pixel, on structured images: k_ssim_fwd / k_ssim_bwd in all eight
operand instantiations and the metrics one, k_alpha_grad, k_exposure_grad.

Yardstick: tests/loss_cases.py — the float64 run of its reference of the whole fused loss.  Bars: per case and per output from the
float32 run of that reference against its float64 run (F = 8; the kernel's output is never used to set one): every gradient
element within F max |g32 - g64| of the case, dE likewise, the SSIM / L1 / MSE values within F (mean |map32 - map64| + one
float32 rounding of the value).  tests/test_cpu_loss_cases.py shows on the CPU that a second float32 evaluation has room under
these bars and that six altered definitions do not.  Every output buffer starts NaN-filled.  Every test prints its ratio
`deviation / bar`; the per-family maxima measured on the MI355X stand in DESIGN.md §16."""
import ctypes as C
import importlib
import math

import pytest
import torch

from tests import loss_cases as lc

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
capi = importlib.import_module("3dgrut_amd._capi")

CASES = [(fam, hw, combo[0]) for fam in lc.FAMILIES for hw in lc.SHAPES for combo in lc.COMBOS]
NAN = float("nan")
bits = lambda t: t.view(torch.int32)
dev = lambda t: None if t is None else t.cuda().contiguous()
nans = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _run(ops, lambda_l1=None, lambda_ssim=None):
    """One call of gut_photometric_loss_run on the operands of a case into NaN-filled outputs: (loss3, d rgba, dE or None)."""
    lib = capi.load()
    H, W = ops["rgba"].shape[:2]
    plane = isinstance(ops["background"], torch.Tensor)
    rgba, gt, B, mask = dev(ops["rgba"]), dev(ops["gt"]), dev(ops["background"]) if plane else None, dev(ops["mask"])
    E = None if ops["exposure"] is None else dev(ops["exposure"].reshape(12))
    need = lib.gut_photometric_workspace_bytes(H, W) if E is None else lib.gut_photometric_exposure_workspace_bytes(H, W)
    ws = nans((need + 3) // 4)
    out3, grad, dE = nans(3), nans(H, W, 4), None if E is None else nans(12)
    ptr = lambda t: None if t is None else t.data_ptr()
    desc = capi.GutPhotometricLoss(rgba.data_ptr(), gt.data_ptr(), ptr(mask), ptr(B), ptr(E), ws.data_ptr(), out3.data_ptr(), grad.data_ptr(),
                                   ptr(dE), 0.0 if plane else float(ops["background"]), ops["lambda_l1"] if lambda_l1 is None else lambda_l1,
                                   ops["lambda_ssim"] if lambda_ssim is None else lambda_ssim)
    rc = lib.gut_photometric_loss_run(C.c_void_p(torch.cuda.current_stream().cuda_stream), H, W, C.byref(desc))
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad, dE


@pytest.mark.parametrize("fam,hw,combo", CASES)
def test_fused_loss_per_element(fam, hw, combo):
    H, W = hw
    c = lc.case(fam, H, W, combo)
    ops = c["ops"]
    out3, grad, dE = _run(ops)
    o, g = out3.cpu(), grad.cpu()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(g).all())            # every element was written
    got = dict(loss=o[0], l1=o[1], ssim=o[2], grad=g, dE=None if dE is None else dE.cpu())
    if dE is not None:
        assert bool(torch.isfinite(got["dE"]).all())
    r = lc.ratios(got, c)
    print(f"\n[loss pixels {fam} {H}x{W} {combo}] deviation / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
          + "; bars " + ", ".join(f"{k} {v:.2e}" for k, v in c["bars"].items() if v is not None and k != "mse"))
    for k, v in r.items():
        assert v <= 1.0, (k, v)
    if ops["mask"] is not None:
        off = ops["mask"] == 0
        assert int(off.sum()) > 0 and bool((g[off] == 0.0).all())                     # all four channels, exactly
    if combo.startswith("black"):
        assert bool((g[..., 3] == 0.0).all())                                         # constant black: no alpha gradient, exactly


@pytest.mark.parametrize("hw", lc.SHAPES)
@pytest.mark.parametrize("combo", [c[0] for c in lc.COMBOS if not c[3]])
def test_tied_elements_get_the_ssim_term_alone(combo, hw):
    """flat_ties without an exposure: where p == q the L1 term adds nothing, so the rgb gradient there is that of a call with
    lambda_l1 = 0 — made at lambda_ssim = 1 and scaled by the ratio of the weights — within the case's gradient bar."""
    H, W = hw
    c = lc.case("flat_ties", H, W, combo)
    ops = c["ops"]
    tied = c["r64"]["abs_map"] == 0
    if ops["mask"] is not None:
        tied &= (ops["mask"] != 0)[..., None]
    assert int(tied.sum()) >= H * W // 2
    _, both, _ = _run(ops)
    _, alone, _ = _run(ops, lambda_l1=0.0, lambda_ssim=1.0)
    a, b = both.cpu()[..., :3].double(), alone.cpu()[..., :3].double() * ops["lambda_ssim"]
    worst = float((a - b)[tied].abs().max())
    l1_step = ops["lambda_l1"] / (3 * H * W)
    print(f"\n[ties {H}x{W} {combo}] {int(tied.sum())} tied elements, largest difference {worst:.3e} (bar {c['bars']['grad']:.3e}; an L1 term "
          f"would add {l1_step:.3e})")
    assert worst <= c["bars"]["grad"]
    assert l1_step > 4 * c["bars"]["grad"]                                           # (on the reference alone: the check can see a sign there)
    assert float((a - b)[~tied].abs().max()) > 0.25 * l1_step                        # and elsewhere the L1 term is in the gradient


def _layout(imgs, layout, fill=None):
    """[2,3,H,W] host images -> (device storage, the [2,3,H,W] view of it the kernels address).  `padded`: the view is the window
    [2:2+H, 3:3+W] of [2,3,H+5,W+7] storage whose padding is NaN."""
    B, Cn, H, W = imgs.shape
    src = imgs if fill is None else torch.full_like(imgs, fill)
    if layout == "nchw":
        store = src.cuda().contiguous()
        return store, store
    if layout == "nhwc_view":
        store = src.permute(0, 2, 3, 1).contiguous().cuda()
        return store, store.permute(0, 3, 1, 2)
    store = nans(B, Cn, H + 5, W + 7)
    view = store[:, :, 2:2 + H, 3:3 + W]
    view.copy_(src.cuda())
    return store, view


@pytest.mark.parametrize("layout", ["nchw", "nhwc_view", "padded"])
@pytest.mark.parametrize("hw", lc.SSIM_SHAPES)
@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_fused_ssim_c_abi_per_element(fam, hw, layout):
    """gut_ssim_forward / gut_ssim_backward on B = 2 independent images (the family's and the next family's) through three
    layouts, into a NaN-filled gradient buffer, with an upstream factor of -2.5; twice, for equal bits."""
    lib = capi.load()
    H, W = hw
    cs = [lc.ssim_case(fam, H, W), lc.ssim_case(lc.FAMILIES[(lc.FAMILIES.index(fam) + 1) % len(lc.FAMILIES)], H, W)]
    _, x = _layout(torch.stack([c["img1"] for c in cs]), layout)
    _, y = _layout(torch.stack([c["img2"] for c in cs]), layout)
    sb, sc, sh, sw = x.stride()
    assert y.stride() == x.stride()
    up = torch.tensor([-2.5], dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        gstore, g = _layout(torch.stack([c["img1"] for c in cs]), layout, fill=NAN)
        assert g.stride() == x.stride()
        out = nans(2)
        ws = nans(2, (lib.gut_ssim_workspace_bytes(3, H, W) + 3) // 4)
        for b in range(2):
            assert lib.gut_ssim_forward(st, 3, H, W, sc, sh, sw, x.data_ptr() + 4 * b * sb, y.data_ptr() + 4 * b * sb, ws[b].data_ptr(),
                                        out[b:].data_ptr()) == 0
            assert lib.gut_ssim_backward(st, 3, H, W, sc, sh, sw, x.data_ptr() + 4 * b * sb, y.data_ptr() + 4 * b * sb, ws[b].data_ptr(),
                                         up.data_ptr(), g.data_ptr() + 4 * b * sb) == 0
        torch.cuda.synchronize()
        return gstore, g, out

    gstore, g, out = launch()
    gstore2, _, out2 = launch()
    assert torch.equal(bits(gstore), bits(gstore2)) and torch.equal(bits(out), bits(out2))     # equal bits, the NaN padding included
    got, s = g.cpu().double(), out.cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(s).all())         # every element of both images was written
    assert int(torch.isnan(gstore).sum()) == gstore.numel() - 2 * 3 * H * W          # and nothing of the padding
    for b, c in enumerate(cs):
        rs = abs(float(s[b]) - c["ssim"]) / c["bar_ssim"]
        rg = float((got[b] - (-2.5) * c["grad"]).abs().max()) / (2.5 * c["bar_grad"])
        print(f"\n[ssim abi {fam} {H}x{W} {layout} image {b}] deviation / bar: ssim {rs:.3f}, grad {rg:.3f}; bars ssim {c['bar_ssim']:.2e}, "
              f"grad {c['bar_grad']:.2e}")
        assert rs <= 1.0 and rg <= 1.0, (b, rs, rg)


@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_fused_ssim_autograd_per_element(fam):
    """losses.fused_ssim on B = 2 images at (27, 21) with an upstream factor of 3: the mean over the two images, each image's
    gradient 3 / 2 times its own."""
    H, W = lc.SSIM_SHAPES[2]
    cs = [lc.ssim_case(fam, H, W), lc.ssim_case(lc.FAMILIES[(lc.FAMILIES.index(fam) + 1) % len(lc.FAMILIES)], H, W)]
    x = torch.stack([c["img1"] for c in cs]).cuda().requires_grad_(True)
    y = torch.stack([c["img2"] for c in cs]).cuda()
    s = losses.fused_ssim(x, y)
    (3.0 * s).backward()
    got = x.grad.cpu().double()
    assert bool(torch.isfinite(got).all())
    rs = abs(float(s.detach()) - 0.5 * (cs[0]["ssim"] + cs[1]["ssim"])) / (0.5 * (cs[0]["bar_ssim"] + cs[1]["bar_ssim"]))
    rg = max(float((got[b] - 1.5 * c["grad"]).abs().max()) / (1.5 * c["bar_grad"]) for b, c in enumerate(cs))
    print(f"\n[ssim autograd {fam}] deviation / bar: ssim {rs:.3f}, grad {rg:.3f}")
    assert rs <= 1.0 and rg <= 1.0


def _psnr_bar(mse, bar_mse):
    """What an MSE within bar_mse of mse can move 10 log10(1 / MSE) by, plus F float32 roundings of the result, as for the values."""
    psnr = 10.0 * math.log10(1.0 / mse)
    return 10.0 * math.log10(mse / (mse - bar_mse)) + lc.F * lc.HALF_ULP * abs(psnr), psnr


@pytest.mark.parametrize("background", ["white", "black"])
@pytest.mark.parametrize("hw", lc.SHAPES)
@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_image_metrics_per_value(fam, hw, background):
    """losses.image_metrics (the kMetrics instantiation): (MSE, PSNR, SSIM, L1) against the float64 run by the scalar bars."""
    H, W = hw
    c = lc.case(fam, H, W, background)
    ops, r64, b = c["ops"], c["r64"], c["bars"]
    out = losses.image_metrics(dev(ops["rgba"]), dev(ops["gt"]), background=background, out=nans(4))
    m = out.cpu().double()
    again = losses.image_metrics(dev(ops["rgba"]), dev(ops["gt"]), background=background, out=nans(4))
    assert torch.equal(bits(out), bits(again))
    if fam == "identical":
        assert float(m[0]) == 0.0 and float(m[1]) == float("inf") and float(m[3]) == 0.0
        assert abs(float(m[2]) - 1.0) <= b["ssim"] + abs(1.0 - float(r64["ssim"]))
    assert bool(torch.isfinite(m[[0, 2, 3]]).all())
    r = dict(mse=abs(float(m[0]) - float(r64["mse"])), ssim=abs(float(m[2]) - float(r64["ssim"])), l1=abs(float(m[3]) - float(r64["l1"])))
    r = {k: (0.0 if v == 0.0 else v / b[k]) for k, v in r.items()}
    if fam != "identical":
        bar, psnr = _psnr_bar(float(r64["mse"]), b["mse"])
        r["psnr"] = abs(float(m[1]) - psnr) / bar
    print(f"\n[metrics {fam} {H}x{W} {background}] deviation / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("hw", lc.SHAPES)
@pytest.mark.parametrize("fam", ["dark", "smooth"])
def test_colour_corrected_metrics_per_value(fam, hw):
    """losses.image_metrics_colour_corrected (the metrics forward with an exposure): the four values against the float64 run of
    the reference under the float64 fit losses.colour_correction, rounded to float32 as the fit kernel rounds its E."""
    H, W = hw
    rgba, gt, _ = lc.family(fam, H, W, 1.0)
    E = losses.colour_correction(lc.composite(rgba.double(), 1.0), gt.double(), ridge=1e-6).float()
    ops = dict(rgba=rgba, gt=gt, background=1.0, exposure=E)
    r64, r32 = lc.reference(**ops, dtype=torch.float64), lc.reference(**ops, dtype=torch.float32)
    b = lc.bars(r32, r64, 0.8, 0.2)
    out, E_got = losses.image_metrics_colour_corrected(dev(rgba), dev(gt), background="white", ridge=1e-6, out=nans(4), exposure_out=nans(3, 4))
    m = out.cpu().double()
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(E_got).all())
    again, E_again = losses.image_metrics_colour_corrected(dev(rgba), dev(gt), background="white", ridge=1e-6, out=nans(4), exposure_out=nans(3, 4))
    assert torch.equal(bits(out), bits(again)) and torch.equal(bits(E_got), bits(E_again))
    bar, psnr = _psnr_bar(float(r64["mse"]), b["mse"])
    r = dict(mse=abs(float(m[0]) - float(r64["mse"])) / b["mse"], psnr=abs(float(m[1]) - psnr) / bar,
             ssim=abs(float(m[2]) - float(r64["ssim"])) / b["ssim"], l1=abs(float(m[3]) - float(r64["l1"])) / b["l1"])
    print(f"\n[cc metrics {fam} {H}x{W}] deviation / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
          + f"; max |E - E64| {float((E_got.cpu() - E).abs().max()):.2e}")
    for k, v in r.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("combo", ["plane+mask+exposure", "grey+mask", "white", "black"])
@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_two_calls_give_equal_bits(fam, combo):
    """The summation order is fixed: loss3, every gradient element and dE."""
    H, W = lc.SHAPES[0]
    ops = lc.case(fam, H, W, combo)["ops"]
    a, b = _run(ops), _run(ops)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(bits(x), bits(y))
