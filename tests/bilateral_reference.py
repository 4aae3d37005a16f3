"""Two references for the bilateral grids of DESIGN.md §21, and the case table both test files run.

(a) the float32 restatement in numpy of the slice, the adjoint (integer sums), the TV term and the Adam step, every operation in
    §21's order, so that the kernels of csrc/gut_bilateral.hip are held to it bit for bit;
(b) the float64 definition: losses.bilateral_slice and losses.bilateral_total_variation under autograd;
and the a-priori bound that holds (a) to (b): the expression of an output evaluated with every operand replaced by its absolute
value and every subtraction by an addition ("sum of |terms|"), times n 2^-24 with n the roundings on the output's longest path.
"""
import importlib

import numpy as np
import torch

F = np.float32
TILE = 16      # the adjoint's workgroup owns a TILE x TILE block of pixels
TABLE = 1024   # 64-bit sums of its LDS table (GUT_BILATERAL_TABLE)
LUM = (F(0.299), F(0.587), F(0.114))
U = 2.0 ** -24


def _losses():
    return importlib.import_module("3dgrut_amd.losses")


# ---------------------------------------------------------------------------------------------------------------- (a) float32
def scales(H, W, Gh, Gw):
    """The two scale factors as the host forms them: float32 divisions, 0 for an axis of one pixel."""
    sx = F(Gw - 1) / F(W - 1) if W > 1 else F(0)
    sy = F(Gh - 1) / F(H - 1) if H > 1 else F(0)
    return F(sx), F(sy)


def _background(background, H, W):
    """[H,W,3] float32 of a constant or a plane."""
    if np.ndim(background) == 0:
        return np.full((H, W, 3), F(background), dtype=F)
    return np.asarray(background, dtype=F).reshape(H, W, 3)


def _axis(s, n):
    fl = np.floor(s)
    f = (s - fl).astype(F)
    i0 = np.clip(fl.astype(np.int64), 0, n - 1)
    return f, i0, np.minimum(i0 + 1, n - 1)


def pixels32(rgba, background, shape):
    """Steps 1 to 3 for every pixel of rgba [H,W,4] under a grid of shape (L, Gh, Gw): dict(comp [P,3], g [P], inside [P],
    wxy [P,4], wz [P,2], w [P,8], xy [P,4] (row * Gw + column), z [P,2], cell [P,8] (z * Gh * Gw + xy), B [P,3])."""
    rgba = np.asarray(rgba, dtype=F)
    H, W = rgba.shape[:2]
    L, Gh, Gw = shape
    B = _background(background, H, W).reshape(-1, 3)
    px = rgba.reshape(-1, 4)
    with np.errstate(all="ignore"):
        alpha1 = (F(1) - px[:, 3:4]).astype(F)
        comp = (px[:, 0:3] + (B * alpha1).astype(F)).astype(F)
        g = (((LUM[0] * comp[:, 0]).astype(F) + (LUM[1] * comp[:, 1]).astype(F)).astype(F) + (LUM[2] * comp[:, 2]).astype(F)).astype(F)
        gc = np.where(np.isnan(g), F(0), np.minimum(np.maximum(g, F(0)), F(1))).astype(F)
        inside = (g > 0) & (g < 1)
    sx, sy = scales(H, W, Gh, Gw)
    xs, ys = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    fx, c0, c1 = _axis((xs.reshape(-1) * sx).astype(F), Gw)
    fy, r0, r1 = _axis((ys.reshape(-1) * sy).astype(F), Gh)
    fz, z0, z1 = _axis((gc * F(L - 1)).astype(F), L)
    wx0, wy0 = (F(1) - fx).astype(F), (F(1) - fy).astype(F)
    wxy = np.stack([wx0 * wy0, fx * wy0, wx0 * fy, fx * fy], axis=1).astype(F)
    wz = np.stack([(F(1) - fz).astype(F), fz], axis=1).astype(F)
    w = np.concatenate([(wxy * wz[:, 0:1]).astype(F), (wxy * wz[:, 1:2]).astype(F)], axis=1)
    xy = np.stack([r0 * Gw + c0, r0 * Gw + c1, r1 * Gw + c0, r1 * Gw + c1], axis=1)
    z = np.stack([z0, z1], axis=1)
    cell = np.concatenate([z[:, 0:1] * (Gh * Gw) + xy, z[:, 1:2] * (Gh * Gw) + xy], axis=1)
    return dict(comp=comp, g=g, inside=inside, wxy=wxy, wz=wz, w=w, xy=xy, z=z, cell=cell, B=B, columns=(c0, c1), rows=(r0, r1))


def gather32(grid, p, derivative=False):
    """A [P,12] (and dA [P,12]): the taps summed left to right, each product rounded on its own."""
    G = np.asarray(grid, dtype=F).reshape(12, -1)
    P = p["comp"].shape[0]
    A = np.zeros((P, 12), dtype=F)
    dA = np.zeros((P, 12), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(12):
            taps = G[k][p["cell"]]                                  # [P,8]
            a = (p["w"][:, 0] * taps[:, 0]).astype(F)
            for n in range(1, 8):
                a = (a + (p["w"][:, n] * taps[:, n]).astype(F)).astype(F)
            A[:, k] = a
            if derivative:
                d = (p["wxy"][:, 0] * (taps[:, 4] - taps[:, 0]).astype(F)).astype(F)
                for n in range(1, 4):
                    d = (d + (p["wxy"][:, n] * (taps[:, 4 + n] - taps[:, n]).astype(F)).astype(F)).astype(F)
                dA[:, k] = d
    return (A, dA) if derivative else A


def _affine(M, c, offset=True):
    """((M0 c0 + M1 c1) + M2 c2) [+ M3], columns of M [P,4] (or [P,3]) against c [P,3]."""
    with np.errstate(all="ignore"):
        out = (((M[:, 0] * c[:, 0]).astype(F) + (M[:, 1] * c[:, 1]).astype(F)).astype(F) + (M[:, 2] * c[:, 2]).astype(F)).astype(F)
        return (out + M[:, 3]).astype(F) if offset else out


def slice32(rgba, background, grid):
    """rgba' [H,W,4] float32: the slice kernel's output."""
    rgba = np.asarray(rgba, dtype=F)
    p = pixels32(rgba, background, np.asarray(grid).shape[1:])
    A = gather32(grid, p)
    out = rgba.copy().reshape(-1, 4)
    for i in range(3):
        out[:, i] = _affine(A[:, 4 * i:4 * i + 4], p["comp"])
    return out.reshape(rgba.shape)


def finite_or_zero(c):
    c = np.asarray(c, dtype=F)
    return np.where(np.isfinite(c), c, F(0)).astype(F)


def scale_exponent(max_bits, pixels):
    """s of the fixed-point unit 2^-s (§20's rule) from the float bits of the magnitude and the number of pixels."""
    if max_bits == 0:
        return 0
    e = max(int(max_bits) >> 23, 1) - 126
    extra = (int(pixels) - 1).bit_length() - 22 if pixels > (1 << 22) else 0
    return min(max(40 - e - extra, -126), 126)


def magnitude_bits(g, comp):
    """The float bits of m = max_pixels max_i |g'_i| max(1, max_j |comp_j| over the finite comp_j), a non-finite product as 0."""
    with np.errstate(all="ignore"):
        gm = np.abs(g).max(axis=1)
        cm = np.maximum(F(1), finite_or_zero(np.abs(comp)).max(axis=1)).astype(F)
        m = finite_or_zero((gm * cm).astype(F))
    return int(np.max(m).astype(F).view(np.uint32)) if m.size else 0


def tv_coefficients(shape):
    """2 / n_axis for x, y, z as float32 divisions (n_axis = 12 times the adjacent pairs along the axis); 0 for a length of 1."""
    L, Gh, Gw = shape
    pairs = ((Gw - 1) * Gh * L, Gw * (Gh - 1) * L, Gw * Gh * (L - 1))
    return [F(2) / F(12 * n) if n > 0 else F(0) for n in pairs]


def tv_term32(grid, lambda_tv):
    """lambda_tv dTV/dG [12,L,Gh,Gw] float32 in the conversion pass's order (what it ADDS is grad + this, see finish32)."""
    return finish32(np.zeros(np.asarray(grid).shape, dtype=F), grid, lambda_tv)


def finish32(grad, grid, lambda_tv):
    """grad + lambda_tv acc, acc = sum over the axes x, y, z of length > 1 of coeff (a - b) from acc = 0; lambda_tv == 0: grad."""
    grad = np.asarray(grad, dtype=F)
    if F(lambda_tv) == 0:
        return grad.copy()
    G = np.asarray(grid, dtype=F)
    coeff = tv_coefficients(G.shape[1:])
    acc = np.zeros(G.shape, dtype=F)
    with np.errstate(all="ignore"):
        for axis, c in zip((3, 2, 1), coeff):
            n = G.shape[axis]
            if n < 2:
                continue
            d = np.diff(G, axis=axis).astype(F)                      # G[i+1] - G[i]
            pad = [(0, 0)] * 4
            pad[axis] = (1, 0)
            a = np.pad(d, pad)                                       # G[c] - G[previous], 0 at the first index
            pad[axis] = (0, 1)
            b = np.pad(d, pad)                                       # G[next] - G[c], 0 at the last
            acc = (acc + (c * (a - b).astype(F)).astype(F)).astype(F)
        return (grad + (F(lambda_tv) * acc).astype(F)).astype(F)


def backward_q(rgba, background, grid, out_grad):
    """(rgba_grad [H,W,4] float32, q int64 [12,L,Gh,Gw], s): the image gradient and the integer sums of the adjoint."""
    rgba, out_grad = np.asarray(rgba, dtype=F), np.asarray(out_grad, dtype=F)
    shape = np.asarray(grid).shape[1:]
    cells = int(np.prod(shape))
    p = pixels32(rgba, background, shape)
    A, dA = gather32(grid, p, derivative=True)
    comp, P = p["comp"], p["comp"].shape[0]
    g = finite_or_zero(out_grad.reshape(-1, 4)[:, 0:3])
    ga = out_grad.reshape(-1, 4)[:, 3]
    with np.errstate(all="ignore"):
        dc = np.stack([_affine(np.stack([A[:, j], A[:, 4 + j], A[:, 8 + j]], axis=1), g, offset=False) for j in range(3)], axis=1)
        d = np.stack([_affine(dA[:, 4 * i:4 * i + 4], comp) for i in range(3)], axis=1)
        D = _affine(g, d, offset=False)
        lm1 = F(shape[0] - 1)
        for j in range(3):
            gamma = F(LUM[j] * lm1)
            dc[:, j] = np.where(p["inside"], (dc[:, j] + (gamma * D).astype(F)).astype(F), dc[:, j])
        da = (-_affine(p["B"], dc, offset=False) + ga).astype(F)
    rgba_grad = np.concatenate([dc, da[:, None]], axis=1).astype(F).reshape(rgba.shape)
    s = scale_exponent(magnitude_bits(g, comp), P)
    assert P * ((1 << 40) + 8) < (1 << 63)                           # int64 holds every total exactly
    scale = np.ldexp(F(1), s).astype(F)
    q = np.zeros((12 * cells,), dtype=np.int64)
    c4 = np.concatenate([comp, np.ones((P, 1), dtype=F)], axis=1)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(4):
                t = finite_or_zero((g[:, i] * c4[:, j]).astype(F))
                for n in range(8):
                    z = np.rint(((p["w"][:, n] * t).astype(F) * scale).astype(F)).astype(np.int64)
                    np.add.at(q, (4 * i + j) * cells + p["cell"][:, n], z)
    return rgba_grad, q.reshape((12,) + tuple(shape)), s


def backward32(rgba, background, grid, out_grad, lambda_tv=0.0):
    """(rgba_grad [H,W,4], grid_grad [12,L,Gh,Gw]) float32 as gut_bilateral_backward writes them."""
    rgba_grad, q, s = backward_q(rgba, background, grid, out_grad)
    grad = (q.astype(F) * np.ldexp(F(1), -s).astype(F)).astype(F)
    return rgba_grad, finish32(grad, grid, lambda_tv)


def adam32(grad, grid, m, v, count, lr, beta1, beta2, eps):
    """One step of gut_bilateral_adam_step in float32 (view_adam_element): returns (grid, m, v, count + 1), new arrays."""
    g, p, m, v = (np.asarray(a, dtype=F) for a in (grad, grid, m, v))
    b1, b2, lr, eps = F(beta1), F(beta2), F(lr), F(eps)
    t = int(count) + 1
    with np.errstate(all="ignore"):
        m = ((b1 * m).astype(F) + ((F(1) - b1).astype(F) * g).astype(F)).astype(F)
        v = ((b2 * v).astype(F) + (((F(1) - b2).astype(F) * g).astype(F) * g).astype(F)).astype(F)
        c1, c2 = F(1.0 - float(b1) ** t), F(1.0 - float(b2) ** t)
        p = (p - ((lr * (m / c1).astype(F)).astype(F) / (np.sqrt((v / c2).astype(F)).astype(F) + eps).astype(F)).astype(F)).astype(F)
    return p, m, v, t


# ---------------------------------------------------------------------------------------------------------------- (b) float64
def comp64(rgba, background):
    rgba = np.asarray(rgba, dtype=F).astype(np.float64)
    H, W = rgba.shape[:2]
    B = _background(background, H, W).astype(np.float64)
    return rgba[..., 0:3] + B * (1.0 - rgba[..., 3:4]), B


def slice64(rgba, background, grid):
    """The rgb part of rgba' [H,W,3] in float64 through losses.bilateral_slice."""
    comp, _ = comp64(rgba, background)
    with torch.no_grad():
        return _losses().bilateral_slice(torch.from_numpy(comp), torch.from_numpy(np.asarray(grid, dtype=F).astype(np.float64))).numpy()


def backward64(rgba, background, grid, out_grad, lambda_tv=0.0):
    """(rgba_grad [H,W,4], grid_grad [12,L,Gh,Gw]) in float64 by autograd: the cotangent's rgb part (non-finite as 0) against the
    slice, its alpha part passed through, lambda_tv TV(G) added to the grid's."""
    losses = _losses()
    og = np.asarray(out_grad, dtype=F)
    g = finite_or_zero(og[..., 0:3]).astype(np.float64)
    comp_np, B = comp64(rgba, background)
    # (a pixel whose colour is not finite: its products g'_i c4_j count as 0 in the grid gradient, and its own image gradient is
    #  outside what the two references are compared on)
    poisoned = ~np.isfinite(comp_np).all(axis=-1)
    comp_np = np.where(poisoned[..., None], 0.0, comp_np)            # guidance 0, c4 = (0, 0, 0, 1): what §21's rules leave of it
    comp = torch.from_numpy(comp_np).requires_grad_(True)
    G = torch.from_numpy(np.asarray(grid, dtype=F).astype(np.float64)).requires_grad_(True)
    total = (losses.bilateral_slice(comp, G) * torch.from_numpy(g)).sum()
    if lambda_tv != 0:
        total = total + float(F(lambda_tv)) * losses.bilateral_total_variation(G)
    total.backward()
    dc = comp.grad.numpy()
    da = -(B * dc).sum(axis=-1) + og[..., 3].astype(np.float64)
    return np.concatenate([dc, da[..., None]], axis=-1), G.grad.numpy()


def branches64(rgba, background, shape):
    """(z0 [P], inside [P]) of the float64 definition: the level piece and the side of the clamp a pixel lies in."""
    comp, _ = comp64(rgba, background)
    c = comp.reshape(-1, 3)
    g = (0.299 * c[:, 0] + 0.587 * c[:, 1]) + 0.114 * c[:, 2]
    with np.errstate(all="ignore"):
        inside = (g > 0) & (g < 1)
        gc = np.where(np.isnan(g), 0.0, np.clip(g, 0.0, 1.0))
    return np.clip(np.floor(gc * (shape[0] - 1)).astype(np.int64), 0, shape[0] - 1), inside


# ------------------------------------------------------------------------------------------------------------- the bound
# Roundings on the longest path of an output, in §21's order (constants 0.299 .. are float32 roundings of the definition's):
#   comp       1 - alpha (1), B alpha1 (1), rgb + . (1)                                                    3
#   g          the constant (1), its product (1), two adds (2)                                         3 + 4 = 7
#   sz, fz, wz gc (L-1) (1), sz - floor (1), 1 - fz (1)                                                      10
#   w_n        wa wb sits at 5 (scale 1, x scale 1, fx 1, 1 - fx 1, product 1); (wa wb) wc (1)               11
#   A_k        w G (1), seven adds (7)                                                                       19
#   out_i      A comp (1), three adds (3)                                                                    23
#   d comp_j   A g' (1), two adds (2) = 22; gamma D sits at 17; the last add (1)                             23
#   d alpha    B d comp (1), two adds (2), + g'_alpha (1)                                                    27
#   grid grad  t = g' c4 (comp 3 + 1 = 4), w t (max(11, 4) + 1 = 12), the conversion of the sum (1)          13
#              and, outside n, half a unit 2^-s per contribution for the rounding to an integer
#   TV term    G - G (1), a - b (1), the coefficient (1) and its product (1), three adds (3), lambda . (1), grad + . (1)   9
N_SLICE, N_IMAGE, N_ALPHA, N_GRID, N_TV = 23, 23, 27, 13, 9


def magnitudes(rgba, background, grid, out_grad=None, lambda_tv=0.0):
    """The sums of |terms| in float64: every expression of §21 with operands replaced by absolute values and subtractions by
    additions, on the taps of the float32 restatement.  dict(out [H,W,3]; with out_grad also image [H,W,4], grid [12,L,Gh,Gw],
    contributions [12,L,Gh,Gw] (products a cell received), unit (2^-s))."""
    rgba = np.asarray(rgba, dtype=F)
    H, W = rgba.shape[:2]
    G = np.abs(np.asarray(grid, dtype=F).astype(np.float64))
    shape = G.shape[1:]
    L, Gh, Gw = shape
    cells = L * Gh * Gw
    p = pixels32(rgba, background, shape)
    px = np.abs(rgba.reshape(-1, 4).astype(np.float64))
    B = np.abs(p["B"].astype(np.float64))
    comp = px[:, 0:3] + B * (1.0 + px[:, 3:4])
    comp = np.where(np.isfinite(comp), comp, 0.0)                    # (a non-finite colour: its products count as 0)
    g = (0.299 * comp[:, 0] + 0.587 * comp[:, 1]) + 0.114 * comp[:, 2]
    g32 = p["g"].astype(np.float64)
    gc = np.where(p["inside"], g, np.where(g32 >= 1, 1.0, 0.0))      # a clamped value is exact
    sx, sy = scales(H, W, Gh, Gw)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))

    def frac(s):
        return s + np.floor(s)
    fx, fy, fz = frac(xs.reshape(-1) * float(sx)), frac(ys.reshape(-1) * float(sy)), frac(gc * (L - 1))
    # (where an axis has one index the fraction is an exact 0 and its complement an exact 1; the general form only loosens)
    wxy = np.stack([(1 + fx) * (1 + fy), fx * (1 + fy), (1 + fx) * fy, fx * fy], axis=1)
    # an exact fraction of 0 leaves weights of exactly 1 and 0: keep the magnitudes at least the weights themselves
    wxy = np.maximum(wxy, p["wxy"].astype(np.float64))
    wz = np.maximum(np.stack([1 + fz, fz], axis=1), p["wz"].astype(np.float64))
    w = np.concatenate([wxy * wz[:, 0:1], wxy * wz[:, 1:2]], axis=1)
    Gf = G.reshape(12, -1)
    taps = np.stack([Gf[k][p["cell"]] for k in range(12)], axis=1)   # [P,12,8]
    A = (taps * w[:, None, :]).sum(axis=2)                           # [P,12]
    c4 = np.concatenate([comp, np.ones((comp.shape[0], 1))], axis=1)
    out = np.stack([(A[:, 4 * i:4 * i + 4] * c4).sum(axis=1) for i in range(3)], axis=1)
    res = dict(out=out.reshape(H, W, 3))
    if out_grad is None:
        return res
    og = np.asarray(out_grad, dtype=F).reshape(-1, 4)
    ga = np.abs(finite_or_zero(og[:, 0:3]).astype(np.float64))
    dA = ((taps[:, :, 0:4] + taps[:, :, 4:8]) * wxy[:, None, :]).sum(axis=2)
    d = np.stack([(dA[:, 4 * i:4 * i + 4] * c4).sum(axis=1) for i in range(3)], axis=1)
    D = (ga * d).sum(axis=1)
    dc = np.stack([A[:, j] * ga[:, 0] + A[:, 4 + j] * ga[:, 1] + A[:, 8 + j] * ga[:, 2] for j in range(3)], axis=1)
    lum = np.array([0.299, 0.587, 0.114])
    dc = dc + np.where(p["inside"], 1.0, 0.0)[:, None] * (lum * (L - 1))[None, :] * D[:, None]
    with np.errstate(all="ignore"):
        da = (B * dc).sum(axis=1) + np.abs(og[:, 3].astype(np.float64))
    res["image"] = np.concatenate([dc, da[:, None]], axis=1).reshape(H, W, 4)
    grid_mag = np.zeros((12 * cells,))
    count = np.zeros((12 * cells,))
    for i in range(3):
        for j in range(4):
            t = ga[:, i] * c4[:, j]
            for n in range(8):
                np.add.at(grid_mag, (4 * i + j) * cells + p["cell"][:, n], w[:, n] * t)
                np.add.at(count, (4 * i + j) * cells + p["cell"][:, n], (t != 0).astype(np.float64))
    res["grid"], res["contributions"] = grid_mag.reshape(G.shape), count.reshape(G.shape)
    s = scale_exponent(magnitude_bits(finite_or_zero(og[:, 0:3]), p["comp"]), comp.shape[0])
    res["unit"] = 2.0 ** -s
    if lambda_tv != 0:
        coeff = [float(c) for c in tv_coefficients(shape)]
        tv = np.zeros(G.shape)
        for axis, c in zip((3, 2, 1), coeff):
            if G.shape[axis] < 2:
                continue
            dsum = G.take(range(1, G.shape[axis]), axis=axis) + G.take(range(0, G.shape[axis] - 1), axis=axis)
            pad = [(0, 0)] * 4
            pad[axis] = (1, 0)
            a = np.pad(dsum, pad)
            pad[axis] = (0, 1)
            tv += c * (a + np.pad(dsum, pad))
        res["tv"] = abs(float(F(lambda_tv))) * tv
    return res


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (H, W, (Gw, Gh, L), background form).  The grid triple is the trainer's order; the arrays are [12, L, Gh, Gw].
CASES = {
    "edges": (23, 37, (5, 4, 3), "one"),
    "edges_plane": (23, 37, (5, 4, 3), "plane"),
    "single_cell": (16, 16, (1, 1, 1), "one"),
    "row": (1, 40, (3, 3, 2), "one"),
    "column": (40, 1, (3, 3, 2), "one"),
    "overflow": (18, 20, (48, 40, 4), "one"),
    "kink": (17, 33, (2, 2, 8), "zero"),
    "shipped": (200, 300, (16, 16, 8), "plane"),
}
NON_FINITE = "edges_plane"   # the case whose cotangent also runs with inf, NaN and exact zeros


def grid_shape(triple):
    """(L, Gh, Gw) of the trainer's (Gw, Gh, L)."""
    return (int(triple[2]), int(triple[1]), int(triple[0]))


def _ulps(v, n):
    """The float32 values from n below v to n above it."""
    bits = int(F(v).view(np.int32))
    return (bits + np.arange(-n, n + 1, dtype=np.int64)).astype(np.int32).view(F)   # positive v: neighbours are neighbouring bits


def _colour(wanted, near):
    """(r, g, b) float32 within 64 ulps of the grey `near` (> 0) whose luminance g, in §21's arithmetic, satisfies wanted(g)."""
    v, blue = np.meshgrid(_ulps(near, 64), _ulps(near, 64), indexing="ij")
    g = (((LUM[0] * v).astype(F) + (LUM[1] * v).astype(F)).astype(F) + (LUM[2] * blue).astype(F)).astype(F)
    hit = np.argwhere(wanted(g))
    if not len(hit):
        raise AssertionError(f"no colour near {near} with the wanted luminance")
    i, j = hit[np.argmin(np.abs(hit - 64).sum(axis=1))]
    return (float(v[i, j]), float(v[i, j]), float(blue[i, j]))


def case(name):
    """dict(rgba [H,W,4], background (float or [H,W,3]), grid [12,L,Gh,Gw], out_grad [H,W,4]) float32, deterministic.  Colours are
    spread so that the luminance leaves [0, 1] on both sides; the grid is the identity plus a smooth-free random part."""
    H, W, triple, bg = CASES[name]
    rng = np.random.default_rng(sum(ord(c) for c in name))
    shape = grid_shape(triple)
    rgba = np.empty((H, W, 4), dtype=F)
    rgba[..., 0:3] = rng.uniform(-0.8, 1.0, (H, W, 3))
    rgba[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    background = {"one": 1.0, "zero": 0.0}.get(bg)
    if background is None:
        background = rng.uniform(0.0, 1.0, (H, W, 3)).astype(F)
    if name == "kink":
        # alpha 1: comp is the colour itself; colours found by search whose luminance is exactly 0, exactly 1, has sz = g (L - 1)
        # exactly k, lies below 0, above 1, and is NaN
        L = shape[0]
        values = [(0.0,) * 3, _colour(lambda g: g == F(1), 1.0), (-0.25,) * 3, (1.5,) * 3, (np.nan,) * 3]
        values += [_colour(lambda g, k=k: (g * F(L - 1)).astype(F) == F(k), k / (L - 1)) for k in range(1, L - 1)]
        flat = rgba.reshape(-1, 4)
        for n, v in enumerate(values * 6):
            flat[3 * n + 1] = v + (1.0,)
    identity = np.zeros((12,) + shape, dtype=F)
    identity[0], identity[5], identity[10] = 1.0, 1.0, 1.0
    grid = (identity + rng.uniform(-0.3, 0.3, identity.shape)).astype(F)
    out_grad = rng.standard_normal((H, W, 4)).astype(F)
    out_grad *= F(1.0 / (H * W))
    return dict(rgba=rgba, background=background, grid=grid, out_grad=out_grad)


def non_finite_cotangent(out_grad):
    """(bad, holes): the cotangent with +-inf, NaN and exact zeros in its rgb part, and the same with those values as 0."""
    holes = np.array(out_grad, dtype=F, copy=True)
    holes[::3, ::5, 0], holes[1::4, ::7, 1], holes[::9, 2::3, 2] = 0.0, 0.0, 0.0
    holes[2::5, 1::4, :3] = 0.0
    bad = holes.copy()
    bad[::3, ::5, 0], bad[1::4, ::7, 1], bad[::9, 2::3, 2] = np.nan, np.inf, -np.inf
    return bad, holes


def footprint(name):
    """The largest number of table entries a 16x16 tile of the case needs: its footprint in columns and rows, times L, times 12."""
    H, W, triple, _ = CASES[name]
    L, Gh, Gw = grid_shape(triple)
    sx, sy = scales(H, W, Gh, Gw)

    def spans(n_pixels, scale, n):
        out = []
        for lo in range(0, n_pixels, TILE):
            hi = min(lo + TILE - 1, n_pixels - 1)
            _, a0, _ = _axis(np.array([F(lo) * scale], dtype=F), n)
            _, _, b1 = _axis(np.array([F(hi) * scale], dtype=F), n)
            out.append(int(b1[0] - a0[0] + 1))
        return out
    return max(spans(W, sx, Gw)) * max(spans(H, sy, Gh)) * L * 12
