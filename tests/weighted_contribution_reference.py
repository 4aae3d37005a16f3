"""The CPU reference of the WEIGHTED contribution walk (gut_trace_contribution_weighted) on the cases of
tests/contribution_reference.py.

`weighted_reference(cam, fwd, plane, params)` is the loop of contribution_reference.reference with every weight multiplied by the
pixel's value of the plane, clamped as the kernel clamps it (a NaN counts as 0): per Gaussian, the sum of w * clamp(plane[py, px]).
`weighted_case(name)` adds, per case, a seeded uniform plane, the reference sums for the plane of ones and for that plane, and the
oracle backward of the cotangent (P, 0, 0, 0): d(sum of P * red)/d(red feature), the independent statement of the weighted sum,
with that call's own flip budget and fp32 conditioning.

Everything is computed once per case and cached: the tests share it and leave it unchanged."""
import functools
import importlib

import numpy as np

from tests import contribution_reference as cr
from tests.common import FLIP_MARGIN_BOUND

oracle = importlib.import_module("oracle.oracle")


def clamp_plane(plane):
    """min(max(e, 0), 1) with a NaN counted as 0, the kernel's clamp on load."""
    p = np.asarray(plane, np.float64)
    return np.where(p > 0, np.minimum(p, 1.0), 0.0)


def weighted_reference(cam, fwd, plane, params=None):
    """The sum of w * clamp(plane[py, px]) per Gaussian, float64 [N]; plane [H,W], or a stack [K,H,W] for [K,N] in one walk."""
    d12, _, _, _, _, W, H = fwd["_inputs"]
    n = d12.shape[0]
    planes = clamp_plane(plane)
    single = planes.ndim == 2
    planes = planes.reshape(-1, H, W)
    out = np.zeros((planes.shape[0], n))
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
            ids = e[acc, 0].astype(np.int64)
            for k in range(planes.shape[0]):
                np.add.at(out[k], ids, w * planes[k, py, px])
    return out[0] if single else out


def random_plane(name, H, W):
    return np.random.default_rng(40 + cr.case_index(name)).uniform(0, 1, (H, W))


@functools.lru_cache(maxsize=None)
def weighted_case(name):
    """dict(plane [H,W] float32, ones_sum [N], weighted_sum [N], feat_grad [N], flip_budget [N], fp32_noise [N]) of the named case."""
    c = cr.case(name)
    cam, fwd, W, H = c["view"]["oracle_cam"], c["ref"], c["W"], c["H"]
    prm = c["params"]()
    plane = random_plane(name, H, W).astype(np.float32)      # what the device reads
    sums = weighted_reference(cam, fwd, np.stack([np.ones((H, W)), plane.astype(np.float64)]), params=prm)
    cot = np.zeros((H, W, 4), np.float32)
    cot[..., 0] = plane
    _, _, feat_g, budget = oracle.backward(cam, fwd, cot, np.zeros((H, W, 1), np.float32), params=prm, flip_bound=FLIP_MARGIN_BOUND)
    return dict(plane=plane, ones_sum=sums[0], weighted_sum=sums[1], feat_grad=feat_g[:, 0].copy(), flip_budget=budget[:, 4].copy(),
                fp32_noise=budget[:, 9].copy())
