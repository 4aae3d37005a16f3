"""The CPU reference of the attribute walk's backward (gut_trace_attributes_bwd) on the cases of
tests/contribution_reference.py, and the reference feature fit of 3dgrut_amd/features.py.

`gradient_reference(cam, fwd, g, params)` is the loop of weighted_contribution_reference.weighted_reference without the clamp:
grad[i, k] = sum over the pixels that accepted Gaussian i of w * g[k, py, px], in float64.  `gradient_case(name)` adds, per case, a
seeded cotangent uniform in [-1, 1] (K = 4), the reference gradient, the independent second statement — the oracle backward's
d(sum of g . colour)/d(colour feature) with the first three planes as the cotangent of the three colour channels — and, per channel,
the flip budget and fp32 conditioning of the oracle backward of the cotangent (g_k, 0, 0, 0), what the device rows are held by.

`fit_case()` is the feature fit on attribute_reference.selection_case() in float64: dense per-view weight matrices from
oracle.debug_ray, planted features, targets W a*, Adam from zero over the two fitted views, the third held out.

Everything is computed once and cached: the tests share it and leave it unchanged."""
import functools
import importlib

import numpy as np

from tests import attribute_reference as ar
from tests import contribution_reference as cr
from tests.common import FLIP_MARGIN_BOUND

oracle = importlib.import_module("oracle.oracle")

K = 4


def gradient_reference(cam, fwd, g, params=None):
    """grad [N,K] float64 with grad[i, k] = the sum over the accepted (pixel, entry) pairs of Gaussian i of w * g[k, py, px];
    g [K,H,W]."""
    d12, _, _, _, _, W, H = fwd["_inputs"]
    n = d12.shape[0]
    g = np.asarray(g, np.float64)
    assert g.ndim == 3 and g.shape[1:] == (H, W)
    out = np.zeros((n, g.shape[0]))
    longest = int((fwd["tile_ranges"][:, 1].astype(np.int64) - fwd["tile_ranges"][:, 0]).max()) if fwd["M"] else 0
    for py in range(H if fwd["M"] else 0):
        for px in range(W):
            e = oracle.debug_ray(cam, fwd, px, py, params=params, max_entries=max(16, longest))
            if not len(e):
                continue
            acc = e[:, 5] != 0
            if not acc.any():
                continue
            t_after = e[acc, 6]
            w = np.concatenate([[1.0], t_after[:-1]]) * e[acc, 3]
            np.add.at(out, e[acc, 0].astype(np.int64), w[:, None] * g[None, :, py, px])
    return out


def weight_matrix(cam, fwd, params=None):
    """The dense matrix W [H*W, N] float64 of blending weights: render(a) = W a per channel, gradient = W^T g."""
    d12, _, _, _, _, W, H = fwd["_inputs"]
    out = np.zeros((H * W, d12.shape[0]))
    longest = int((fwd["tile_ranges"][:, 1].astype(np.int64) - fwd["tile_ranges"][:, 0]).max()) if fwd["M"] else 0
    for py in range(H if fwd["M"] else 0):
        for px in range(W):
            e = oracle.debug_ray(cam, fwd, px, py, params=params, max_entries=max(16, longest))
            if not len(e):
                continue
            acc = e[:, 5] != 0
            if not acc.any():
                continue
            t_after = e[acc, 6]
            w = np.concatenate([[1.0], t_after[:-1]]) * e[acc, 3]
            np.add.at(out[py * W + px], e[acc, 0].astype(np.int64), w)
    return out


def random_cotangent(name, H, W, k=K):
    return np.random.default_rng(110 + cr.case_index(name)).uniform(-1, 1, (k, H, W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gradient_case(name):
    """dict(g float32 [4,H,W], grad float64 [N,4], feat_grad [N,3] with flip_budget3 / fp32_noise3 [N] (the second statement and its
    own budget), flip_budget [4][N], fp32_noise [4][N] (per channel, of the cotangent (g_k, 0, 0, 0))) of the named case."""
    c = cr.case(name)
    cam, fwd, W, H = c["view"]["oracle_cam"], c["ref"], c["W"], c["H"]
    prm = c["params"]()
    g = random_cotangent(name, H, W)                 # what the device reads
    grad = gradient_reference(cam, fwd, g.astype(np.float64), params=prm)
    zero_dist = np.zeros((H, W, 1), np.float32)
    cot = np.zeros((H, W, 4), np.float32)
    cot[..., :3] = g[:3].transpose(1, 2, 0)
    _, _, feat_g, budget3 = oracle.backward(cam, fwd, cot, zero_dist, params=prm, flip_bound=FLIP_MARGIN_BOUND)
    budgets, noises = [], []
    for k in range(K):
        cot = np.zeros((H, W, 4), np.float32)
        cot[..., 0] = g[k]
        _, _, _, b = oracle.backward(cam, fwd, cot, zero_dist, params=prm, flip_bound=FLIP_MARGIN_BOUND)
        budgets.append(b[:, 4].copy())
        noises.append(b[:, 9].copy())
    return dict(g=g, grad=grad, feat_grad=feat_g[:, :3].copy(), flip_budget3=budget3[:, 4].copy(), fp32_noise3=budget3[:, 9].copy(),
                flip_budget=budgets, fp32_noise=noises)


# ---- the reference fit ----
FIT_LR, FIT_ITERATIONS = 0.03, 200


def planted_features(positions):
    """a* = (sin 2x, cos 1.5y, z, [x < 0]) of the Gaussians' positions, float64 [N,4]."""
    p = np.asarray(positions, np.float64)
    return np.stack([np.sin(2.0 * p[:, 0]), np.cos(1.5 * p[:, 1]), p[:, 2], (p[:, 0] < 0).astype(np.float64)], axis=1)


def adam_fit(matrices, targets, n, k, lr=FIT_LR, iterations=FIT_ITERATIONS):
    """torch.optim.Adam's update (beta 0.9 / 0.999, eps 1e-8) in float64 from zero on mean((W_v a - target_v)^2), views round-robin."""
    a, m, v = np.zeros((n, k)), np.zeros((n, k)), np.zeros((n, k))
    for it in range(iterations):
        Wv, t = matrices[it % len(matrices)], targets[it % len(matrices)]
        grad = Wv.T @ (2.0 * (Wv @ a - t) / t.size)
        m = 0.9 * m + 0.1 * grad
        v = 0.999 * v + 0.001 * grad * grad
        a = a - lr * (m / (1.0 - 0.9 ** (it + 1))) / (np.sqrt(v / (1.0 - 0.999 ** (it + 1))) + 1e-8)
    return a


@functools.lru_cache(maxsize=None)
def fit_case():
    """attribute_reference.selection_case()'s scene and three views (two fitted, one held out).  dict(scene, views, matrices [3]
    [H*W,N], planted [N,4], rendered [3][4,H,W] (W a*), alphas [3][H,W] (W 1), maps [3][4,H,W] (the un-premultiplied target maps
    rendered / alpha, 0 where alpha is 0: alpha * map = W a*), fitted [N,4], heldout_mse, zero_mse, seen [N] bool)."""
    c = ar.selection_case()
    Wd, Hd = ar.SELECTION_SIZE
    n = c["d12"].shape[0]
    matrices = [weight_matrix(v["oracle_cam"], f) for v, f in zip(c["views"], c["fwds"])]
    planted = planted_features(c["scene"]["positions"])
    flat = [Wv @ planted for Wv in matrices]                       # [H*W, 4]
    fitted = adam_fit(matrices[:2], flat[:2], n, 4)
    rendered = [t.T.reshape(4, Hd, Wd) for t in flat]
    alphas = [Wv.sum(1).reshape(Hd, Wd) for Wv in matrices]
    maps = [np.where(al[None] > 0, r / np.where(al[None] > 0, al[None], 1.0), 0.0) for r, al in zip(rendered, alphas)]
    mse = lambda a: float(((matrices[2] @ a - flat[2]) ** 2).mean())
    seen = (matrices[0].sum(0) > 0) | (matrices[1].sum(0) > 0)
    return dict(scene=c["scene"], views=c["views"], matrices=matrices, planted=planted, rendered=rendered, alphas=alphas, maps=maps,
                fitted=fitted, heldout_mse=mse(fitted), zero_mse=mse(np.zeros((n, 4))), seen=seen)
