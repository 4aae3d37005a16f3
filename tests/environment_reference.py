"""The cube-map background of DESIGN.md §20 twice on the CPU: a float32 restatement, op by op in the kernels' order (numpy does not
contract), which the GPU tests compare bit for bit, and a float64 definition of the same sampling and adjoint, which says how far the
restatement is from the mathematics.  Test infrastructure: nothing here is imported by the package."""
import math

import numpy as np

F = np.float32
TILE = 16   # the adjoint's workgroup owns a TILE x TILE block of pixels


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' rotation about `axis` by `angle` radians, float64 [3,3]."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def pinhole_rays(height, width, fov_degrees):
    """Unit directions [H,W,3] float32 of a pinhole camera looking along +z, `fov_degrees` across the width, pixel centres."""
    f = 0.5 * width / math.tan(math.radians(fov_degrees) / 2.0)
    x = (np.arange(width, dtype=np.float64) + 0.5 - 0.5 * width) / f
    y = (np.arange(height, dtype=np.float64) + 0.5 - 0.5 * height) / f
    d = np.stack([np.broadcast_to(x[None, :], (height, width)), np.broadcast_to(y[:, None], (height, width)),
                  np.ones((height, width))], axis=-1)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)


def fisheye_rays(size, fov_degrees):
    """An equidistant fisheye's ray table [size,size,3] float32: the angle from +z grows linearly with the radius, `fov_degrees`
    across the width; the corners lie beyond it and are kept (they reach still further round)."""
    c = (np.arange(size, dtype=np.float64) + 0.5 - 0.5 * size) / (0.5 * size)
    x, y = np.meshgrid(c, c, indexing="xy")
    r = np.sqrt(x * x + y * y)
    theta = r * math.radians(fov_degrees) / 2.0
    s = np.where(r > 0, np.sin(theta) / np.where(r > 0, r, 1.0), 0.0)
    return np.stack([s * x, s * y, np.cos(theta)], axis=-1).astype(F)


def case(name):
    """(rays [H,W,3] float32, M [3,3] float32, R) of the issue's cases a..d and of the fisheye table `f`."""
    if name in ("a", "b"):
        return pinhole_rays(48, 64, 90.0), rotation((1, 1, 1), 0.9553).astype(F), 8 if name == "a" else 512
    if name == "c":
        return pinhole_rays(40, 40, 150.0), rotation((0.3, 1, 0.2), 0.7).astype(F), 16
    if name == "d":
        return pinhole_rays(48, 64, 60.0), rotation((0, 1, 0), 0.3).astype(F), 1
    if name == "f":
        return fisheye_rays(40, 180.0), rotation((1, 0.2, 0.1), 0.5).astype(F), 16
    raise KeyError(name)


CASES = ("a", "b", "c", "d")


# ---- float32, op by op ----------------------------------------------------------------------------------------------------------------
def taps32(rays, M, R):
    """(valid [P] bool, face [P], texel [P,4] linear index face R^2 + row R + column, w [P,4] float32) in the order 00, 10, 01, 11
    (w_ab: column a, row b).  Void pixels have valid False and zeros."""
    d = np.ascontiguousarray(rays, dtype=F).reshape(-1, 3)
    M = np.asarray(M, dtype=F).reshape(3, 3)
    with np.errstate(all="ignore"):
        e = np.stack([(M[i, 0] * d[:, 0] + M[i, 1] * d[:, 1]) + M[i, 2] * d[:, 2] for i in range(3)], axis=1)
        assert e.dtype == F
        a = np.abs(e)
        finite = np.isfinite(e).all(axis=1)
        axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
        rows = np.arange(d.shape[0])
        m = a[rows, axis]
        valid = finite & (m != 0)
        ms = np.where(valid, m, F(1))
        es = np.where(valid[:, None], e, F(0))
        face = 2 * axis + (es[rows, axis] < 0)
        u = es[rows, (axis + 1) % 3] / ms
        v = es[rows, (axis + 2) % 3] / ms
        half = F(0.5) * F(R)
        s = (u + F(1)) * half - F(0.5)
        t = (v + F(1)) * half - F(0.5)
        fi, fj = np.floor(s), np.floor(t)
        fx, fy = s - fi, t - fj
        assert fx.dtype == F and u.dtype == F and s.dtype == F
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    c0, c1 = np.clip(i0, 0, R - 1), np.clip(i0 + 1, 0, R - 1)
    r0, r1 = np.clip(j0, 0, R - 1), np.clip(j0 + 1, 0, R - 1)
    wx0, wy0 = F(1) - fx, F(1) - fy
    w = np.stack([wx0 * wy0, fx * wy0, wx0 * fy, fx * fy], axis=1)
    base = face * R * R
    texel = np.stack([base + r0 * R + c0, base + r0 * R + c1, base + r1 * R + c0, base + r1 * R + c1], axis=1)
    w = np.where(valid[:, None], w, F(0)).astype(F)
    texel = np.where(valid[:, None], texel, 0)
    return valid, np.where(valid, face, 0), texel, w


def sample32(rays, M, texels):
    """The plane [H,W,3] float32 of the map texels [6,R,R,3]: ((w00 T00 + w10 T10) + w01 T01) + w11 T11, +0 for a void pixel."""
    R = texels.shape[1]
    T = np.ascontiguousarray(texels, dtype=F).reshape(-1, 3)
    valid, _, texel, w = taps32(rays, M, R)
    b = ((w[:, 0:1] * T[texel[:, 0]] + w[:, 1:2] * T[texel[:, 1]]) + w[:, 2:3] * T[texel[:, 2]]) + w[:, 3:4] * T[texel[:, 3]]
    assert b.dtype == F
    b = np.where(valid[:, None], b, F(0))
    return b.reshape(rays.shape[:-1] + (3,))


def finite_or_zero(c):
    c = np.asarray(c, dtype=F)
    return np.where(np.isfinite(c), c, F(0))


def cotangent_from_rgba(rgba, rgba_grad):
    """c = (1 - alpha) g_rgb in float32: 1 - alpha rounded first, then each product; [H,W,3]."""
    rgba, g = np.asarray(rgba, dtype=F), np.asarray(rgba_grad, dtype=F)
    with np.errstate(all="ignore"):
        return (F(1) - rgba[..., 3:4]) * g[..., 0:3]


def scale_exponent(max_bits, pixels):
    """s of the fixed-point unit 2^-s from the float bits of the largest finite |c| and the number of pixels."""
    if max_bits == 0:
        return 0
    e = max(int(max_bits) >> 23, 1) - 126
    extra = (int(pixels) - 1).bit_length() - 22 if pixels > (1 << 22) else 0   # ceil(log2(pixels)) - 22
    return min(max(40 - e - extra, -126), 126)


def max_abs_bits(c):
    c = np.abs(finite_or_zero(c))
    return int(np.max(c).astype(F).view(np.uint32)) if c.size else 0


def adjoint_q(rays, M, R, c, pixels=None):
    """(q int64 [6,R,R,3], s): the integer sums of the products w c_k, each rounded to float32, scaled by 2^s and rounded to nearest
    even.  `pixels` overrides the pixel count the exponent sees."""
    c = finite_or_zero(c).reshape(-1, 3)
    valid, _, texel, w = taps32(rays, M, R)
    s = scale_exponent(max_abs_bits(c), c.shape[0] if pixels is None else pixels)
    scale = np.ldexp(F(1), s).astype(F)
    q = np.zeros((6 * R * R, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        for n in range(4):
            p = (w[:, n:n + 1] * c).astype(F)
            z = np.rint(p * scale).astype(np.int64)
            np.add.at(q, texel[valid, n], z[valid])
    return q.reshape(6, R, R, 3), s


def adjoint32(rays, M, R, c, pixels=None):
    """The gradient [6,R,R,3] float32 as the conversion pass writes it: float(q) 2^-s."""
    q, s = adjoint_q(rays, M, R, c, pixels)
    return (q.astype(F) * np.ldexp(F(1), -s).astype(F)).astype(F)


def distinct_texels_per_tile(rays, M, R, c=None):
    """The number of distinct texels each TILE x TILE pixel tile touches with a non-zero weight (and, with c, a non-zero cotangent)."""
    H, W = rays.shape[:2]
    valid, _, texel, w = taps32(rays, M, R)
    live = valid[:, None] & (w != 0)
    if c is not None:
        live &= (finite_or_zero(c).reshape(-1, 3) != 0).any(axis=1)[:, None]
    texel, live = texel.reshape(H, W, 4), live.reshape(H, W, 4)
    counts = []
    for y in range(0, H, TILE):
        for x in range(0, W, TILE):
            counts.append(len(np.unique(texel[y:y + TILE, x:x + TILE][live[y:y + TILE, x:x + TILE]])))
    return counts


# ---- float64, the definition ------------------------------------------------------------------------------------------------------------
def taps64(rays, M, R):
    d = np.asarray(rays, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        e = d @ M.T
        a = np.abs(e)
        finite = np.isfinite(e).all(axis=1)
        axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
        rows = np.arange(d.shape[0])
        m = a[rows, axis]
        valid = finite & (m != 0)
        ms = np.where(valid, m, 1.0)
        es = np.where(valid[:, None], e, 0.0)
        face = 2 * axis + (es[rows, axis] < 0)
        s = (es[rows, (axis + 1) % 3] / ms + 1.0) * (0.5 * R) - 0.5
        t = (es[rows, (axis + 2) % 3] / ms + 1.0) * (0.5 * R) - 0.5
    fi, fj = np.floor(s), np.floor(t)
    fx, fy = s - fi, t - fj
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    c0, c1 = np.clip(i0, 0, R - 1), np.clip(i0 + 1, 0, R - 1)
    r0, r1 = np.clip(j0, 0, R - 1), np.clip(j0 + 1, 0, R - 1)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=1)
    base = face * R * R
    texel = np.stack([base + r0 * R + c0, base + r0 * R + c1, base + r1 * R + c0, base + r1 * R + c1], axis=1)
    return valid, np.where(valid, face, 0), np.where(valid[:, None], texel, 0), np.where(valid[:, None], w, 0.0)


def sample64(rays, M, texels):
    R = texels.shape[1]
    T = np.asarray(texels, dtype=np.float64).reshape(-1, 3)
    _, _, texel, w = taps64(rays, M, R)
    b = sum(w[:, n:n + 1] * T[texel[:, n]] for n in range(4))
    return b.reshape(rays.shape[:-1] + (3,))


def adjoint64(rays, M, R, c):
    c = np.asarray(c, dtype=np.float64)
    c = np.where(np.isfinite(c), c, 0.0).reshape(-1, 3)
    _, _, texel, w = taps64(rays, M, R)
    g = np.zeros((6 * R * R, 3))
    for n in range(4):
        np.add.at(g, texel[:, n], w[:, n:n + 1] * c)
    return g.reshape(6, R, R, 3)
