"""The fused loss restated once, its structured test images and the bars they are held to (CPU only).  Shared by
tests/test_cpu_loss_cases.py (the reference, the margins, the bars and the proof that they bite, without a device) and
tests/test_gpu_loss_pixels.py (the kernels of csrc/gut_ssim.hip, per pixel).

reference(): the whole fused loss in plain torch at a dtype of choice,
    image = mask * (E [rgb + B (1 - alpha); 1])   against   mask * gt,
    loss = lambda_l1 * mean |image - gt| + lambda_ssim * (1 - mean SSIM over the valid region),
with losses.apply_exposure and the operations of train.ssim (its window, its constants, its order), so that in float64 it IS
losses.photometric_loss — tests/test_cpu_loss_cases.py holds it to tests/test_gpu_exposure_loss._case — and returns, next to the
loss, L1, SSIM, d rgba and dE, the per-pixel SSIM map and the |p - q| map before their means.  `variant` alters one rule of the
definition (VARIANTS); variants only ever play the part of a wrong kernel.

scheme32(): a second, independent float32 evaluation — the derivative-map scheme of k_ssim_fwd / k_ssim_bwd in torch: separable
pass, e - mu^2, the three maps, the adjoint blur, then A^T g, the alpha slot and the twelve sums — which tells whether a bar is too
tight for a correct float32 kernel before any device is involved.

Families (family()): noise (torch.rand, what every older loss test uses: the control), dark, flat_ties, smooth, identical,
out_of_range.  Shapes: (37, 85) = 6 x 3 = 18 tiles, where xcd_tile permutes (full = 2) and leaves a tail of 2, both dimensions have
partial tiles and the bottom tile row has no valid SSIM pixel; (12, 17), two tiles, two valid rows; for fused_ssim also (27, 21),
whose right-hand tile holds border pixels only.

Bars (bars()): from the float32 run of reference() against its float64 run and from nothing else, per case and per output:
    gradient elements (d rgba, alpha included)   |got - g64| <= F max |g32 - g64|      one number per case
    dE                                           the same rule over its 12 entries
    SSIM, L1, MSE                                F (mean over pixels |map32 - map64| + 2^-24 |value64|)
    loss                                         lambda_l1 * L1 bar + lambda_ssim * SSIM bar
The first term of a value's bar bounds what the maps' float32 rounding can move the mean by.  It can be zero although the value is
not: torch.rand draws multiples of 2^-24, so over constant black |p - q| of `noise` is exact in float32 per pixel, and so is that of
`smooth` (p within a factor 2 of q) — but no float32 evaluation states the mean of 9435 such numbers exactly: it adds them in float32
(the kernels: 256 per workgroup by a butterfly, the partials then in double) and rounds the result.  The second term is the smallest
error such an evaluation can be credited with, one rounding of the value to float32, and F covers the rest as it does everywhere.
F = 8: two independent float32 evaluations of one definition (torch autograd and scheme32) differ in their worst gradient
element by a factor 0.56 .. 2.49 over these families, shapes and operands (dE: 0.23 .. 1.82); a kernel adds fma contraction and a third summation order.  A kernel beyond 8 is a
finding.  Where a float64 map is identically zero (|p - q| of `identical` without an exposure) the float32 map is too, the bar is
0 and the check is the exact one: the output must be 0.0f.

Decision margin (margin()): the sign of p - q is the one discontinuous rule of the loss.  Over all elements of a case |p - q| in
float64 is exactly 0 or at least 1e-6 (the float32 image differs from it by less than 5e-7), so float32 and float64 take the same
branch everywhere and nothing is left out of a comparison.  Ties are exact by construction: every value that takes part in one is
a multiple of 1/8 (flat_ties) or 1/256 (identical) in rgba, plane and mask, which float32 — through the kernel's fmaf too — and
float64 carry without rounding.  An exposure would round differently in the two: with one, flat_ties and identical run with
lambda_l1 = 0, lambda_ssim = 1, where no decision is taken."""
import functools
import importlib

import torch
import torch.nn.functional as Fn

from tests.test_gpu_masked_loss import _mask as _mask_37

losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")

F = 8.0
MARGIN = 1e-6
HALF_ULP = 2.0 ** -24   # of a float32 in [1, 2), relative: what rounding ONE result to float32 costs
HALO = 5
SHAPES = [(37, 85), (12, 17)]
SSIM_SHAPES = SHAPES + [(27, 21)]
FAMILIES = ["noise", "dark", "flat_ties", "smooth", "identical", "out_of_range"]
E_TEST = torch.tensor([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.03], [0.02, -0.05, 1.20, 0.04]], dtype=torch.float32)
GREY = 0.5      # the constant background of the eight combinations: unlike 1.0 it shows a lost factor in the alpha gradient

# (name, constant background or "plane", mask, exposure): mask x plane x exposure, then constant white and constant black alone, and
# black once more under a mask and an exposure (the per-pixel pass's da = 0 branch)
COMBOS = [(f"{'plane' if plane else 'grey'}{'+mask' if mask else ''}{'+exposure' if exp else ''}", "plane" if plane else GREY, mask, exp)
          for plane in (False, True) for mask in (False, True) for exp in (False, True)]
COMBOS += [("white", 1.0, False, False), ("black", 0.0, False, False), ("black+mask+exposure", 0.0, True, True)]
COMBO = {c[0]: c for c in COMBOS}

VARIANTS = {"c1=9e-4": dict(c1=9e-4), "c1=0": dict(c1=0.0), "c2=1e-4": dict(c2=1e-4), "tie=+1": dict(tie=1.0), "valid=4": dict(valid=4),
            "halo_mask=centre": dict(halo_mask="centre")}

# The seed of a family at a shape: the first at which the decision margin holds in all eleven combinations and the second float32
# evaluation stays within F / 2 of every bar (find_seed below; tests/test_cpu_loss_cases.py asserts both).  1 where not listed.
SEEDS = {("smooth", 37, 85): 2}


def mask_for(H, W):
    """(37, 85): the pattern of tests/test_gpu_masked_loss.py (an edge inside a tile and its neighbours' halo, a hole across the
    x = 32 tile border, one column at 0.5).  (12, 17): columns < 6 zero, column 11 at 0.5."""
    if W > 45:
        return _mask_37(H, W)
    m = torch.ones((H, W), dtype=torch.float32)
    m[:, :6] = 0.0
    m[:, 11] = 0.5
    return m


def composite(rgba, B):
    """rgb + B (1 - alpha) in rgba's dtype; B a number or an [H,W,3] plane."""
    return rgba[..., :3] + B * (1.0 - rgba[..., 3:])


def _split(target, alpha, B):
    """The rgba whose composite over B is `target` (up to float32 rounding)."""
    return torch.cat([target - B * (1.0 - alpha), alpha], dim=-1).float().contiguous()


def _rectangles(H, W, g):
    """Flat rectangles on an empty ground: (colour [H,W,3], alpha [H,W,1]) in multiples of 1/8.  The rectangles cross the tile
    borders at x = 16, 32, 48, 64, 80 and y = 16, 32 where the shape has them, and overlap."""
    colour = torch.zeros((H, W, 3))
    alpha = torch.zeros((H, W, 1))
    boxes = [(2, 9, 3, 14), (6, 12, 10, 17)] if W <= 17 else [(3, 22, 5, 30), (12, 20, 26, 52), (14, 35, 44, 70), (0, 37, 60, 67),
                                                              (28, 37, 10, 85), (5, 11, 76, 85)]
    for (y0, y1, x0, x1) in boxes:
        colour[y0:y1, x0:x1] = torch.randint(1, 9, (3,), generator=g).float() / 8.0
        alpha[y0:y1, x0:x1] = float(torch.randint(4, 9, (1,), generator=g)) / 8.0
    return colour, alpha


@functools.lru_cache(maxsize=None)
def family(name, H, W, background):
    """(rgba [H,W,4], gt [H,W,3], plane [H,W,3] or None) of one family, float32, from a fixed seed.  background: a number, or
    "plane".  Only flat_ties and identical depend on it through more than the plane: their gt is the composite."""
    seed = SEEDS.get((name, H, W), 1)
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(s, generator=g)
    plane = background == "plane"
    if name == "noise":
        rgba, gt, B = rand(H, W, 4), rand(H, W, 3), rand(H, W, 3)
    elif name == "dark":
        alpha, B = 1.0 - 0.05 * rand(H, W, 1), 0.05 * rand(H, W, 3)
        pred, gt = 0.05 * rand(H, W, 3), 0.05 * rand(H, W, 3)
        rgba = _split(pred, alpha, B if plane else background)
    elif name == "flat_ties":
        B = torch.randint(0, 9, (H, W, 3), generator=g).float() / 8.0
        rgb, alpha = _rectangles(H, W, g)
        gt = composite(torch.cat([rgb, alpha], -1), B if plane else background)       # exact in float32
        off = torch.zeros((H, W, 1), dtype=torch.bool)
        off[:, :W // 2] = True                                                         # the half that does not tie: the left one
        rgba = torch.cat([torch.where(off, 0.97 * rgb + 0.01, rgb), alpha], -1)
    elif name == "smooth":
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        gt = torch.stack([0.5 + 0.4 * torch.sin((x + 5.0 * k) / 9.0) * torch.cos((y + 3.0 * k) / 7.0) for k in range(3)], -1)
        alpha, B = rand(H, W, 1), rand(H, W, 3)
        rgba = _split(gt + 0.01 * torch.randn((H, W, 3), generator=g), alpha, B if plane else background)
    elif name == "identical":
        rgba = torch.randint(0, 257, (H, W, 4), generator=g).float() / 256.0
        B = torch.randint(0, 257, (H, W, 3), generator=g).float() / 256.0
        gt = composite(rgba.double(), B.double() if plane else background).float()      # multiples of 2^-16 below 2: exact
    elif name == "out_of_range":
        alpha, B = rand(H, W, 1), rand(H, W, 3)
        pred, gt = rand(H, W, 3) * 1.6 - 0.3, rand(H, W, 3) * 1.2 - 0.1
        rgba = _split(pred, alpha, B if plane else background)
    else:
        raise KeyError(name)
    return rgba.float().contiguous(), gt.float().contiguous(), (B.float().contiguous() if plane else None)


def _blur(x, window):
    c = x.shape[1]
    wh = window.view(1, 1, 1, -1).expand(c, 1, 1, -1)
    wv = window.view(1, 1, -1, 1).expand(c, 1, -1, 1)
    return Fn.conv2d(Fn.conv2d(x, wh, groups=c), wv, groups=c)


def ssim_map(img1, img2, c1=0.01 ** 2, c2=0.03 ** 2, centre_mask=None):
    """The per-pixel SSIM of train.ssim, operation for operation, before its mean: [B,C,H-10,W-10].  centre_mask (variant
    halo_mask="centre"): img1 and img2 come unmasked and every window takes the mask value at its centre."""
    window = train._gauss_window(device=img1.device, dtype=img1.dtype)
    mu1, mu2 = _blur(img1, window), _blur(img2, window)
    e11, e22, e12 = _blur(img1 * img1, window), _blur(img2 * img2, window), _blur(img1 * img2, window)
    if centre_mask is not None:
        mu1, mu2 = mu1 * centre_mask, mu2 * centre_mask
        e11, e22, e12 = e11 * centre_mask ** 2, e22 * centre_mask ** 2, e12 * centre_mask ** 2
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    return ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))


def reference(rgba, gt, background=0.0, mask=None, exposure=None, lambda_l1=0.8, lambda_ssim=0.2, dtype=torch.float64, variant=None):
    """The fused loss of one view and its gradients by autograd, at `dtype`.  rgba [H,W,4], gt [H,W,3]; background a number or an
    [H,W,3] plane; mask None or [H,W]; exposure None or [3,4] / [12].  variant: None or a key of VARIANTS.
    Returns a dict of detached tensors of that dtype: loss, l1, ssim, mse (0-d); grad [H,W,4]; dE [12] or None; ssim_map
    [3,H-10,W-10]; abs_map and sq_map [H,W,3] (|p - q| and its square, the masked images); p, q [H,W,3]."""
    v = VARIANTS[variant] if variant is not None else {}
    H, W = rgba.shape[:2]
    x = rgba.detach().to(dtype).requires_grad_(True)
    B = background.to(dtype) if isinstance(background, torch.Tensor) else float(background)
    E = None if exposure is None else exposure.detach().to(dtype).reshape(3, 4).requires_grad_(True)
    q = gt.detach().to(dtype)
    p = composite(x, B)
    if E is not None:
        p = losses.apply_exposure(p, E)
    p_open, q_open = p, q
    if mask is not None:
        m = mask.to(dtype)[..., None]
        p, q = p * m, q * m
    chw = lambda t: t.permute(2, 0, 1)[None]
    if v.get("halo_mask") == "centre" and mask is not None:
        smap = ssim_map(chw(p_open), chw(q_open), centre_mask=mask.to(dtype)[None, None, HALO:H - HALO, HALO:W - HALO])
    else:
        border = HALO - v.get("valid", HALO)            # variant valid=4: the map one pixel wider, over the zero-padded image
        pad = lambda t: Fn.pad(t, (border,) * 4) if border else t
        smap = ssim_map(pad(chw(p)), pad(chw(q)), c1=v.get("c1", 0.01 ** 2), c2=v.get("c2", 0.03 ** 2))
    ssim = smap.mean() if "valid" not in v else smap.sum() / (3 * (H - 2 * HALO) * (W - 2 * HALO))
    amap = (p - q).abs()
    l1 = amap.mean()
    if "tie" in v:                                       # the value of |.| with the subgradient v["tie"] where p == q
        l1 = l1 + (v["tie"] * (p - p.detach()) * (p.detach() == q)).sum() / amap.numel()
    loss = lambda_l1 * l1 + lambda_ssim * (1.0 - ssim)
    loss.backward()
    d = lambda t: t.detach()
    return dict(loss=d(loss), l1=d(l1), ssim=d(ssim), mse=d((amap * amap).mean()), grad=x.grad, dE=None if E is None else E.grad.reshape(12),
                ssim_map=d(smap)[0] if "valid" not in v else d(smap)[0][:, border:-border, border:-border], abs_map=d(amap), sq_map=d(amap * amap),
                p=d(p), q=d(q))


def _blur_hw(x, window):
    """[C,H,W] -> [C,H-10,W-10], horizontal pass first, as the kernels do."""
    return _blur(x[None], window)[0]


def scheme32(rgba, gt, background=0.0, mask=None, exposure=None, lambda_l1=0.8, lambda_ssim=0.2):
    """The same loss in float32 the way k_ssim_fwd / k_ssim_bwd / k_exposure_grad / k_alpha_grad compute it, without autograd:
    the three derivative maps of the SSIM with respect to mu1, sigma1^2 and sigma12, zero on the border, blurred with the window
    (the adjoint of the valid blur), g = scale (a + 2 p b + q d) + l1 weight * sign(p - q), times the mask, then A^T g, the alpha
    slot -sum_k B_k d_k and dE = [sum g_c comp_k | sum g_c].  The means are taken in double from the float32 maps, as the finish
    kernels do.  Returns reference()'s dict (float32 tensors; loss, l1, ssim, mse as float64 0-d)."""
    f32 = torch.float32
    H, W = rgba.shape[:2]
    x = rgba.detach().to(f32)
    B = background.to(f32) if isinstance(background, torch.Tensor) else float(background)
    comp = composite(x, B)
    E = None if exposure is None else exposure.detach().to(f32).reshape(3, 4)
    p = comp if E is None else losses.apply_exposure(comp, E)
    q = gt.detach().to(f32)
    m = None if mask is None else mask.to(f32)[..., None]
    if m is not None:
        p, q = p * m, q * m
    P, Q = p.permute(2, 0, 1), q.permute(2, 0, 1)
    w = train._gauss_window(dtype=f32)
    mu1, mu2 = _blur_hw(P, w), _blur_hw(Q, w)
    e11, e22, e12 = _blur_hw(P * P, w), _blur_hw(Q * Q, w), _blur_hw(P * Q, w)
    C1, C2 = 0.0001, 0.0009
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sg1, sg2, sg12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, Bq, Cc, D = mu1_sq + mu2_sq + C1, sg1 + sg2 + C2, 2.0 * mu12 + C1, 2.0 * sg12 + C2
    smap = (Cc * D) / (A * Bq)
    d_mu1 = (mu2 * 2.0 * D) / (A * Bq) - (mu2 * 2.0 * Cc) / (A * Bq) - (mu1 * 2.0 * Cc * D) / (A * A * Bq) + (mu1 * 2.0 * Cc * D) / (A * Bq * Bq)
    d_s1 = (-Cc * D) / (A * Bq * Bq)
    d_s12 = (2.0 * Cc) / (A * Bq)
    adj = lambda t: _blur_hw(Fn.pad(t, (2 * HALO,) * 4), w)            # zero border, then the (symmetric) window: [C,H,W]
    a, b, d = adj(d_mu1), adj(d_s1), adj(d_s12)
    count, numel = 3 * (H - 2 * HALO) * (W - 2 * HALO), 3 * H * W
    scale = torch.tensor(-lambda_ssim, dtype=f32) * torch.tensor(1.0 / count, dtype=f32)
    g = scale * (a + 2.0 * P * b + Q * d)
    if lambda_l1 != 0.0:
        g = g + torch.tensor(lambda_l1 / numel, dtype=f32) * torch.sign(P - Q)
    g = g.permute(1, 2, 0)
    if m is not None:
        g = g * m
    drgb = g if E is None else g @ E[:, :3]                           # d_k = sum_c A[c][k] g_c
    dalpha = -(drgb * B).sum(-1, keepdim=True) if isinstance(B, torch.Tensor) else -B * drgb.sum(-1, keepdim=True)
    dE = None
    if E is not None:
        dE = torch.cat([torch.einsum("hwc,hwk->ck", g, comp), g.sum((0, 1))[:, None]], 1).reshape(12)
    amap = (p - q).abs()
    l1, ssim = amap.double().mean(), smap.double().mean()
    return dict(loss=lambda_l1 * l1 + lambda_ssim * (1.0 - ssim), l1=l1, ssim=ssim, mse=(amap * amap).double().mean(),
                grad=torch.cat([drgb, dalpha], -1), dE=dE, ssim_map=smap, abs_map=amap, sq_map=amap * amap, p=p, q=q)


def weights(fam, exposure):
    """(lambda_l1, lambda_ssim) of a case: the trainer's 0.8 / 0.2, but with an exposure the two families made of ties run on the
    SSIM term alone (float32 and float64 would break the ties differently)."""
    return (0.0, 1.0) if exposure and fam in ("flat_ties", "identical") else (0.8, 0.2)


def operands(fam, H, W, combo):
    """The CPU operands of one case as keyword arguments of reference() / scheme32()."""
    _, background, masked, exposure = COMBO[combo]
    rgba, gt, plane = family(fam, H, W, background)
    l1, ls = weights(fam, exposure)
    return dict(rgba=rgba, gt=gt, background=plane if plane is not None else background, mask=mask_for(H, W) if masked else None,
                exposure=E_TEST if exposure else None, lambda_l1=l1, lambda_ssim=ls)


def bars(r32, r64, lambda_l1, lambda_ssim):
    """The bars of one case from its two runs of reference(): dict(grad, dE (None without an exposure), ssim, l1, mse, loss)."""
    dev = lambda k: (r32[k].double() - r64[k]).abs()
    value = lambda k, v: F * (float(dev(k).mean()) + HALF_ULP * abs(float(r64[v])))
    b = dict(grad=F * float(dev("grad").max()), dE=None if r64["dE"] is None else F * float(dev("dE").max()),
             ssim=value("ssim_map", "ssim"), l1=value("abs_map", "l1"), mse=value("sq_map", "mse"))
    b["loss"] = lambda_l1 * b["l1"] + lambda_ssim * b["ssim"]
    return b


def margin(r64):
    """The smallest non-zero |p - q| of a float64 run (inf if all tie)."""
    a = r64["abs_map"]
    return float(a[a > 0].min()) if bool((a > 0).any()) else float("inf")


@functools.lru_cache(maxsize=None)
def case(fam, H, W, combo):
    """One case, computed once and shared, not modified: the operands, both runs of the reference and the bars."""
    ops = operands(fam, H, W, combo)
    r64 = reference(**ops, dtype=torch.float64)
    r32 = reference(**ops, dtype=torch.float32)
    return dict(fam=fam, H=H, W=W, combo=combo, ops=ops, r64=r64, r32=r32, bars=bars(r32, r64, ops["lambda_l1"], ops["lambda_ssim"]),
                margin=margin(r64))


def ratios(got, c):
    """How far an evaluation `got` (reference()'s keys; tensors or numbers) lies from the float64 run of case c, in units of the
    case's bars: dict(grad, dE, ssim, l1, loss), each `deviation / bar`, so <= 1 passes.  A zero bar gives 0 for an exact match and
    inf otherwise."""
    r64, b = c["r64"], c["bars"]
    div = lambda e, bar: (0.0 if e == 0.0 else float("inf")) if bar == 0.0 else e / bar
    out = dict(grad=div(float((got["grad"].double() - r64["grad"]).abs().max()), b["grad"]))
    if r64["dE"] is not None:
        out["dE"] = div(float((got["dE"].double() - r64["dE"]).abs().max()), b["dE"])
    for k in ("ssim", "l1", "loss"):
        out[k] = div(abs(float(got[k]) - float(r64[k])), b[k])
    return out


def ssim_case_images(fam, H, W):
    """fused_ssim's operands of a family: (img1, img2) [3,H,W] float32 — the family's prediction over black and its ground truth."""
    rgba, gt, _ = family(fam, H, W, 0.0)
    return composite(rgba, 0.0).permute(2, 0, 1).contiguous(), gt.permute(2, 0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def ssim_case(fam, H, W):
    """mean SSIM and d(mean SSIM) / d img1 of a family at one shape, with their bars: reference() on the opaque image with
    lambda_l1 = 0, lambda_ssim = 1, whose loss is 1 - SSIM."""
    img1, img2 = ssim_case_images(fam, H, W)
    rgba = torch.cat([img1.permute(1, 2, 0), torch.ones((H, W, 1))], -1)
    ops = dict(rgba=rgba, gt=img2.permute(1, 2, 0), lambda_l1=0.0, lambda_ssim=1.0)
    r64, r32 = reference(**ops, dtype=torch.float64), reference(**ops, dtype=torch.float32)
    b = bars(r32, r64, 0.0, 1.0)
    return dict(img1=img1, img2=img2, ssim=float(r64["ssim"]), grad=-r64["grad"][..., :3].permute(2, 0, 1).contiguous(),
                bar_ssim=b["ssim"], bar_grad=F * float((r32["grad"][..., :3].double() - r64["grad"][..., :3]).abs().max()))


def find_seed(name, H, W, first=1, tries=400):
    """The first seed at which family `name` keeps the decision margin in every combination and the second float32 evaluation
    stays within F / 2 of every bar — what tests/test_cpu_loss_cases.py asserts, on the CPU alone (how SEEDS was filled)."""
    for seed in range(first, first + tries):
        SEEDS[(name, H, W)] = seed
        family.cache_clear()
        case.cache_clear()
        ok = True
        for combo in COMBO:
            c = case(name, H, W, combo)
            if (c["ops"]["lambda_l1"] != 0.0 and c["margin"] < MARGIN) or max(ratios(scheme32(**c["ops"]), c).values()) > 0.5:
                ok = False
                break
        if ok:
            return seed
    raise RuntimeError(f"no seed for {name} {H}x{W}")
