"""The CPU reference of the surface walk (gut_trace_surface) on the cases of tests/contribution_reference.py, float64.

Per pixel, oracle.debug_ray gives the accepted entries, their alpha and T after; w = T_before * alpha as everywhere.  The oracle
does not hand out the per-entry hit distance, so `hit_distances` recomputes it on the host from the [N,12] rows, the view's c2w and
the pixel's ray:

    gro = R^T (o - mu) / s,   grd = normalize(R^T d / s),   hit_t = | s * grd (grd . -gro) |

(quaternion wxyz, R its textbook rotation).  tests/test_cpu_surface.py earns the formula first: sum of w * hit_t per pixel must
reproduce the oracle's own `dist` plane.

`level_planes(name, level)` and `max_weight_planes(name)` are the two modes with, per pixel, whether the pixel is NEAR — whether
another valid fp32 evaluation may choose differently there, see `slack`.  `wall_*` is the scene of the point-cloud test.

Everything is computed once and cached: the tests share it and leave it unchanged."""
import functools
import importlib

import numpy as np

from tests import contribution_reference as cr
from tests.common import COLOUR_TOL, PIX_FLIP, ROW_FLIP_BOUND, cams, make_view

oracle = importlib.import_module("oracle.oracle")

LEVELS = (0.5, 0.1, 0.9)


def quat_rotation(q):
    """[n,3,3] float64 rotations of [n,4] wxyz quaternions (normalised here)."""
    q = np.asarray(q, np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def world_ray(view, px, py):
    """(origin, unit direction) of pixel (px, py) in the world, float64."""
    c2w = np.asarray(view["c2w"], np.float64)
    o = c2w[:3, :3] @ np.asarray(view["ro"], np.float64).reshape(view["H"], view["W"], 3)[py, px] + c2w[:3, 3]
    d = c2w[:3, :3] @ np.asarray(view["rd"], np.float64).reshape(view["H"], view["W"], 3)[py, px]
    return o, d


def hit_distances(d12, ids, o, d):
    """hit_t [k] float64 of the rows `ids` of d12 for the world ray (o, d)."""
    rows = np.asarray(d12, np.float64)[ids]
    mu, s = rows[:, 0:3], rows[:, 8:11]
    R = quat_rotation(rows[:, 4:8])
    gro = np.einsum("kji,kj->ki", R, o[None] - mu) / s
    grd = np.einsum("kji,j->ki", R, d) / s
    grd /= np.linalg.norm(grd, axis=1, keepdims=True)
    proj = -(grd * gro).sum(1)
    return np.linalg.norm(s * grd * proj[:, None], axis=1)


@functools.lru_cache(maxsize=None)
def surface_case(name):
    """The named case of contribution_reference with, per pixel in row-major order, the accepted entries `entries[p]` = (ids int64,
    w, t_after, hit_t, their positions in the pixel's walked list), the plane `dist_sum` [H,W] = sum of w * hit_t, and `slack` [H,W] = COLOUR_TOL + PIX_FLIP x the pixel's
    flip budget (oracle.render_margins(..., budget_bound=ROW_FLIP_BOUND)): how far another valid fp32 evaluation may move a
    transmittance or a weight of the pixel (the selection test's precedent)."""
    c = cr.case(name)
    return _surface_of(c["view"], c["ref"], c["d12"], c["params"]())


def _surface_of(view, fwd, d12, prm):
    cam, W, H = view["oracle_cam"], view["W"], view["H"]
    empty = (np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.int64))
    entries, dist_sum = [], np.zeros((H, W))
    longest = int((fwd["tile_ranges"][:, 1].astype(np.int64) - fwd["tile_ranges"][:, 0]).max()) if fwd["M"] else 0
    for py in range(H):
        for px in range(W):
            e = oracle.debug_ray(cam, fwd, px, py, params=prm, max_entries=max(16, longest)) if fwd["M"] else np.zeros((0, 8))
            acc = e[:, 5] != 0 if len(e) else np.zeros(0, bool)
            if not acc.any():
                entries.append(empty)
                continue
            ids, t_after = e[acc, 0].astype(np.int64), e[acc, 6]
            w = np.concatenate([[1.0], t_after[:-1]]) * e[acc, 3]
            hit_t = hit_distances(d12, ids, *world_ray(view, px, py))
            entries.append((ids, w, t_after, hit_t, np.nonzero(acc)[0]))
            dist_sum[py, px] = float((w * hit_t).sum())
    _, budget = oracle.render_margins(cam, fwd, params=prm, budget_bound=ROW_FLIP_BOUND)
    slack = COLOUR_TOL + PIX_FLIP * budget[..., 0].astype(np.float64)
    hit = np.array([len(e[0]) > 0 for e in entries]).reshape(H, W)
    return dict(view=view, fwd=fwd, d12=d12, W=W, H=H, entries=entries, dist_sum=dist_sum, slack=slack, hit=hit)


def _surface(key):
    """surface_case(key), or wall_surface(i) for the key "wall:i"."""
    return wall_surface(int(key[5:])) if key.startswith("wall:") else surface_case(key)


def _planes(s, choose, near_of):
    H, W = s["H"], s["W"]
    dist, wgt, ids = np.zeros((H, W)), np.zeros((H, W)), np.full((H, W), -1, np.int64)
    near, pos = np.zeros((H, W), bool), np.full((H, W), -1, np.int64)
    for p, (e_ids, w, t_after, hit_t, list_pos) in enumerate(s["entries"]):
        if not len(e_ids):
            continue
        py, px = divmod(p, W)
        k = choose(w, t_after)
        if k is not None:
            dist[py, px], wgt[py, px], ids[py, px], pos[py, px] = hit_t[k], w[k], e_ids[k], list_pos[k]
        near[py, px] = near_of(w, t_after, s["slack"][py, px])
    return dict(distance=dist, id=ids, weight=wgt, near=near, position=pos)


@functools.lru_cache(maxsize=None)
def _level_planes(key, level):
    s = _surface(key)

    def choose(w, t_after):
        below = np.nonzero(t_after < level)[0]
        return int(below[0]) if len(below) else None
    return _planes(s, choose, lambda w, t_after, slack: bool((np.abs(t_after - level) <= slack).any()))


def level_planes(name, level):
    """dict(distance, id (-1: none), weight, near, position (of the chosen entry in the pixel's walked list)) [H,W]: per pixel
    the first accepted entry after which T < level.  near: some accepted entry has |T_after - level| <= slack(p)."""
    return _level_planes(name, float(level))


@functools.lru_cache(maxsize=None)
def _max_weight_planes(key):
    s = _surface(key)

    def near_of(w, t_after, slack):
        top = np.sort(w)[::-1]
        return bool(len(top) > 1 and top[0] - top[1] <= 2.0 * slack)
    return _planes(s, lambda w, t_after: int(np.argmax(w)), near_of)      # (argmax: the first of equal weights)


def max_weight_planes(name):
    """The same planes for the accepted entry of the largest weight.  near: the two largest weights differ by at most 2 slack(p)."""
    return _max_weight_planes(name)


# ---- the wall: a plane of discs, seen from three sides, whose level-0.5 points must lie on it ----
WALL_SIZE = (64, 48)
WALL_POSES = ((0.0, 0.0, -3.0), (1.4, 0.3, -2.8), (-1.2, -0.8, -2.9))


@functools.lru_cache(maxsize=None)
def wall_scene():
    """A jittered 18 x 14 grid (252 rows) of flat, mostly opaque discs on z = 0: radius 0.12 to 0.2 in the plane (neighbours at
    0.16 overlap), thickness 0.002, the thin axis within a few degrees of z, density 0.9 to 0.99."""
    rng = np.random.default_rng(18)
    gx, gy = np.meshgrid(np.arange(18), np.arange(14))
    n = gx.size
    pos = np.stack([(gx.ravel() - 8.5) * 0.16, (gy.ravel() - 6.5) * 0.16, np.zeros(n)], 1)
    pos[:, :2] += rng.uniform(-0.04, 0.04, (n, 2))
    tilt = rng.normal(0.0, 0.02, (n, 2))          # small rotations about x and y: (w, x, y, z) ~ (1, tx / 2, ty / 2, 0)
    quat = np.concatenate([np.ones((n, 1)), 0.5 * tilt, np.zeros((n, 1))], 1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    scale = np.concatenate([rng.uniform(0.12, 0.2, (n, 2)), np.full((n, 1), 0.002)], 1)
    sph = np.zeros((n, 16, 3))
    sph[:, 0, :] = rng.uniform(-1.0, 1.0, (n, 3))
    return dict(positions=pos.astype(np.float32), rotation=quat.astype(np.float32), scale=scale.astype(np.float32),
                density=rng.uniform(0.9, 0.99, (n, 1)).astype(np.float32), features=sph.reshape(n, 48).astype(np.float32))


@functools.lru_cache(maxsize=None)
def wall_views():
    W, H = WALL_SIZE
    return tuple(make_view("pinhole", W, H, cams.look_at_c2w(eye, (0.0, 0.0, 0.0)), fx=1.0 * W) for eye in WALL_POSES)


@functools.lru_cache(maxsize=None)
def wall_surface(i):
    scenes = importlib.import_module("3dgrut_amd.scenes")
    sc, view = wall_scene(), wall_views()[i]
    d12 = np.ascontiguousarray(scenes.pack_density(sc))
    fwd = oracle.forward(view["oracle_cam"], view["W"], view["H"], d12, np.ascontiguousarray(sc["features"]), view["ro"], view["rd"], sh_degree=3)
    return _surface_of(view, fwd, d12, None)


def backproject(view, distance):
    """[H,W,3] float64 world points origin + distance x unit direction; NaN where distance is 0."""
    c2w = np.asarray(view["c2w"], np.float64)
    H, W = view["H"], view["W"]
    o = np.asarray(view["ro"], np.float64).reshape(H, W, 3) @ c2w[:3, :3].T + c2w[:3, 3]
    d = np.asarray(view["rd"], np.float64).reshape(H, W, 3) @ c2w[:3, :3].T
    dist = np.where(np.asarray(distance, np.float64) > 0, distance, np.nan)
    return o + dist[..., None] * d


@functools.lru_cache(maxsize=None)
def wall_points():
    """dict(points [P,3], max_abs_z, max_distance): the reference's level-0.5 points of the three wall views."""
    pts, far = [], 0.0
    for i in range(len(WALL_POSES)):
        planes = level_planes(f"wall:{i}", 0.5)
        p = backproject(wall_views()[i], planes["distance"])[planes["id"] >= 0]
        pts.append(p)
        far = max(far, float(planes["distance"].max()))
    pts = np.concatenate(pts)
    return dict(points=pts, max_abs_z=float(np.abs(pts[:, 2]).max()), max_distance=far)
