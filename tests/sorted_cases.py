"""Cases for the sorted variant of the compositor (render.splat.k_buffer_size = K; gut_render_sorted.hip), shared by
tests/test_cpu_sorted_cases.py (every precondition, on the CPU oracle alone), tests/test_cpu_oracle.py (the two-evaluation band of
the k-buffer model) and tests/test_gpu_sorted_variant.py (the same cases on the device).

Both sorted kernels stage a tile's list kStage = 256 entries at a time and carry each ray's k-buffer across the reloads, so a hit
found in one chunk may be composited while a later chunk is walked, or in the drain after the last one.  The cases:

  * single_tile(255 / 256 / 257 / 513 / 1025): one 16 x 16 tile whose list has exactly that many entries
    (capacity_cases.single_tile_list): one staging, one staging to the last slot, and one, two and four reloads;
  * terminating_deep_list(): the same tile with a larger opaque share: rays fall below min_transmittance while a later chunk is
    walked and hits are still pending in their buffers, which the drain must then NOT composite;
  * geometry_clones(): Gaussians replaced by 2 - 4 clones of bit-equal position, rotation and scale but different density and
    colour: their hit distances are bit-equal in every evaluation, so the composite order among them is decided by the insertion
    rule (`t > stored`, bubbling from the back) and the list order alone;
  * order_pairs(): pairs of Gaussians whose centres are a few ulps apart along the view direction: order decisions within fp32
    noise are common (the scene the noise estimate of the hit distance is measured on);
  * rays_from_a_centre_plane(): rays that start in the centre plane of a large Gaussian: its hit distance is exactly zero, which is
    all the range test `hit_t > tmin` ever rejects inside the scene box;
  * existing(name): c1_pinhole_128, ragged_100x70, fisheye_144x96, inside_cloud, dense_big_splats as tests/test_gpu_parity.CASES
    defines them (restated here: that module needs a device).

A case is a dict: the ACTIVATED rows `d12` [N,12] / `sph` [N,48] exactly as both the oracle and the device get them (no model, no
activation in between), the view, W, H, the oracle's forward result `ref` and its parameters.  kbuffer(case, K, ...) caches the
oracle's k-buffer render of a case.  No list here has padding ids inside its range (the overflow path is not the subject)."""
import functools
import importlib

import numpy as np

from tests import capacity_cases as cc
from tests.common import cams, make_view, scenes

oracle = importlib.import_module("oracle.oracle")

K_STAGE = 256          # list entries per staging of k_render_sorted / k_render_sorted_backward (kBlock)
K_MAX = 16             # kKMax


def _finish(name, d12, sph, view, W, H, params=None, sh_degree=3):
    prm = params() if params is not None else oracle.default_params()
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=sh_degree, params=prm)
    assert ref["M"] > 0 and not (ref["sorted_ids"] == 0xFFFFFFFF).any(), "no padding ids inside a list"
    return dict(name=name, d12=d12, sph=sph, view=view, W=W, H=H, ref=ref, sh_degree=sh_degree,
                params=params if params is not None else oracle.default_params, _kb={})


def _from_scene(name, sc, kind, W, H, eye, tgt, kw, params=None):
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    return _finish(name, np.ascontiguousarray(scenes.pack_density(sc)), np.ascontiguousarray(sc["features"].astype(np.float32)), view, W, H, params)


def _big():
    sc = scenes.scene_c1(400, 7)
    sc["scale"] = (sc["scale"] * 4.0).astype(np.float32)
    sc["density"] = np.clip(sc["density"] * 1.5, 0, 0.999).astype(np.float32)
    return sc


EXISTING = {
    "c1_pinhole_128": (lambda: scenes.scene_c1(1000, 0), "pinhole", 128, 128, ((0, 0, -4), (0, 0, 0)), dict(fx=128)),
    "ragged_100x70": (lambda: scenes.scene_c1(700, 3), "pinhole", 100, 70, ((0.5, -0.3, -3.0), (0, 0.1, 0)), dict(fx=90, fy=95)),
    "fisheye_144x96": (lambda: scenes.scene_c1(900, 5), "fisheye", 144, 96, ((0.1, 0.0, -1.5), (0, 0, 0.5)), dict()),
    "inside_cloud": (lambda: scenes.scene_c1(1500, 6), "pinhole", 96, 96, ((0.05, 0.02, -0.1), (0, 0, 1)), dict(fx=60)),
    "dense_big_splats": (_big, "pinhole", 64, 64, ((0, 0, -3), (0, 0, 0)), dict(fx=64)),
}


@functools.lru_cache(maxsize=None)
def existing(name, negative_colours=False, **overrides):
    """One of the five scenes of tests/test_gpu_parity.CASES.  negative_colours: a third of the Gaussians get a negative SH dc term
    (the scene of test_sorted_variant_reference_backward, on which the two forms of the sorted backward differ).  overrides: oracle
    parameters away from their defaults (kernel_degree=..., max_alpha=..., ...)."""
    mk, kind, W, H, (eye, tgt), kw = EXISTING[name]
    sc = mk()
    if negative_colours:
        sc["features"] = sc["features"].copy()
        sc["features"][::3, 0:3] -= 2.5
    params = None
    if overrides:
        def params():
            prm = oracle.default_params()
            for k, v in overrides.items():
                assert hasattr(prm, k), k
                setattr(prm, k, v)
            return prm
    tag = "".join(f"/{k}={v}" for k, v in overrides.items()) + ("/negative" if negative_colours else "")
    return _from_scene(name + tag, sc, kind, W, H, eye, tgt, kw, params)


def from_rows(name, d12, sph, view, W, H, **overrides):
    """A case from activated rows a test already has (tests/test_gpu_parity.py builds them through the model's activations)."""
    params = None
    if overrides:
        def params():
            prm = oracle.default_params()
            for k, v in overrides.items():
                assert hasattr(prm, k), k
                setattr(prm, k, v)
            return prm
    return _finish(name, np.ascontiguousarray(d12, np.float32), np.ascontiguousarray(sph, np.float32), view, W, H, params)


@functools.lru_cache(maxsize=None)
def single_tile(length):
    c = cc.single_tile_list(length)
    return _finish(f"single_tile_{length}", c["d12"], c["sph"], c["view"], 16, 16)


TERMINATING_LENGTH, TERMINATING_OPAQUE_SHARE, TERMINATING_OPAQUE = 1025, 0.5, 0.7


@functools.lru_cache(maxsize=None)
def terminating_deep_list():
    """single_tile(1025)'s rows with the opaque share raised from 2 % to TERMINATING_OPAQUE_SHARE (density TERMINATING_OPAQUE): the
    footprints grow with the density, so the list gets longer (3336 entries, 14 stagings); a third of the rays lose their transmittance
    while a later chunk is walked."""
    c = cc.single_tile_list(TERMINATING_LENGTH)
    d12 = c["d12"].copy()
    rng = np.random.default_rng(97)
    d12[:, 3] = np.where(rng.random(d12.shape[0]) < TERMINATING_OPAQUE_SHARE, TERMINATING_OPAQUE, d12[:, 3]).astype(np.float32)
    case = _finish("terminating_deep_list", d12, c["sph"], c["view"], 16, 16)
    return case


CLONE_GROUPS = (2, 3, 4, 2, 3, 4)


def _clone_scene(reverse):
    sc = scenes.scene_c1(300, 17)
    rng = np.random.default_rng(171)
    # parents: large, fairly opaque Gaussians near the axis, so that each group covers many pixels with a weight that matters
    parents = np.argsort(np.linalg.norm(sc["positions"][:, :2], axis=1))[:len(CLONE_GROUPS)]
    rows, group = [{k: v.copy() for k, v in sc.items()}], [np.full(300, -1)]
    keep = np.setdiff1d(np.arange(300), parents)
    rows[0] = {k: v[keep] for k, v in rows[0].items()}
    group[0] = group[0][keep]
    for g, (m, p) in enumerate(zip(CLONE_GROUPS, parents)):
        cl = {k: np.repeat(v[p:p + 1], m, axis=0).copy() for k, v in sc.items()}
        cl["scale"][:] = np.float32(0.22)
        cl["density"][:, 0] = np.linspace(0.35, 0.6, m).astype(np.float32)
        cl["features"][:] = 0.0
        for j in range(m):                                   # saturated, mutually different colours: dc term only
            cl["features"][j, (g + j) % 3] = 1.6
            cl["features"][j, (g + j + 1) % 3] = -1.6
        if reverse:
            cl = {k: v[::-1].copy() for k, v in cl.items()}
        rows.append(cl)
        group.append(np.full(m, g))
    out = {k: np.concatenate([r[k] for r in rows]) for k in sc}
    return out, np.concatenate(group)


@functools.lru_cache(maxsize=None)
def geometry_clones(reverse=False):
    """reverse=True: the same scene with the clones of every group stored in reverse: bit-equal depth keys are listed by particle id,
    so the list order of every group is reversed, and with it the composite order."""
    sc, group = _clone_scene(reverse)
    case = _from_scene("geometry_clones" + ("_reversed" if reverse else ""), sc, "pinhole", 64, 64, (0, 0, -4), (0, 0, 0), dict(fx=64))
    case["group"] = group
    return case


@functools.lru_cache(maxsize=None)
def rays_from_a_centre_plane():
    """The range test `hit_t > tmin`: tmin is 0 for every ray inside the scene box and hit_t is a norm, so the test only ever rejects a
    hit distance of exactly zero — a ray that STARTS in the plane through a Gaussian's centre perpendicular to it.  Gaussian 0 is a
    large axis-aligned splat at (0, 0, 2) in front of the identity-pose camera; every ray starts where the pinhole ray of its pixel
    pierces the plane z = 2 and runs along +z, so for Gaussian 0 every product of grd . gro is exactly zero in any evaluation, on the
    oracle and on the device.  Its response passes on most of the image; it is composited nowhere."""
    W = H = 64
    fx = 64.0
    sc = scenes.scene_c1(300, 31)
    sc["positions"][:, 2] += np.float32(3.5)           # the rest of the scene lies behind the plane
    sc["positions"][0] = (0.0, 0.0, 2.0)
    sc["rotation"][0] = (1.0, 0.0, 0.0, 0.0)
    sc["scale"][0] = 0.5
    sc["density"][0] = 0.8
    sc["features"][0] = 0.0
    sc["features"][0, 0:3] = (1.7, -1.7, 1.7)
    view = dict(make_view("pinhole", W, H, np.eye(4, dtype=np.float32), fx=fx))
    ro, rd = np.zeros_like(view["ro"]), np.zeros_like(view["rd"])
    r3, d3 = ro.reshape(H, W, 3), rd.reshape(H, W, 3)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    r3[..., 0] = (xs + np.float32(0.5) - np.float32(W / 2)) / np.float32(fx) * np.float32(2.0)
    r3[..., 1] = (ys + np.float32(0.5) - np.float32(H / 2)) / np.float32(fx) * np.float32(2.0)
    r3[..., 2] = 2.0
    d3[..., 2] = 1.0
    view["ro"], view["rd"] = ro, rd
    return _finish("rays_from_a_centre_plane", np.ascontiguousarray(scenes.pack_density(sc)), np.ascontiguousarray(sc["features"].astype(np.float32)),
                   view, W, H)


ORDER_PAIRS = 12


@functools.lru_cache(maxsize=None)
def order_pairs():
    """scene_c1(600) at 96 x 96 in which ORDER_PAIRS Gaussians are followed by a twin whose centre is 1 - 4 ulps farther along the
    view direction (everything else of the geometry equal; density and colour differ): on the pixels both cover, their hit distances
    agree to within fp32 noise and are not bit-equal, so the order is decided by rounding."""
    sc = scenes.scene_c1(600, 23)
    rng = np.random.default_rng(231)
    first = rng.permutation(600)[:ORDER_PAIRS]
    twin = {k: v[first].copy() for k, v in sc.items()}
    z = twin["positions"][:, 2].copy()
    for j in range(ORDER_PAIRS):
        for _ in range(1 + j % 4):
            z[j] = np.nextafter(z[j], np.float32(np.inf))
    twin["positions"][:, 2] = z
    twin["density"] = np.clip(1.0 - twin["density"], 0.05, 0.9).astype(np.float32)
    twin["features"] = (-twin["features"]).astype(np.float32)
    out = {k: np.concatenate([sc[k], twin[k]]) for k in sc}
    case = _from_scene("order_pairs", out, "pinhole", 96, 96, (0, 0, -4), (0, 0, 0), dict(fx=96))
    case["pairs"] = np.stack([first, 600 + np.arange(ORDER_PAIRS)], 1)
    return case


# ---- the oracle's k-buffer render of a case, and what the preconditions read from it ------------------------------------------
def kbuffer(case, K, budget_bound=None):
    key = (K, budget_bound)
    if key not in case["_kb"]:
        count = oracle.render_kbuffer(case["view"]["oracle_cam"], case["ref"], K=K, params=case["params"]())["order_count"]
        max_order = int(count.max()) + 1
        case["_kb"][key] = oracle.render_kbuffer(case["view"]["oracle_cam"], case["ref"], K=K, params=case["params"](), max_order=max_order,
                                                 margins=True, budget_bound=budget_bound)
        assert int(case["_kb"][key]["order_count"].max()) <= max_order
    return case["_kb"][key]


def list_positions(case, kb):
    """[P,L] int: the position within its tile's list of every composited entry (-1 where the order is padded)."""
    ref, W, H = case["ref"], case["W"], case["H"]
    gx = (W + 15) // 16
    ids = kb["order_ids"]
    pos = np.full(ids.shape, -1, np.int64)
    N = case["d12"].shape[0]
    for tile, (b, e) in enumerate(ref["tile_ranges"]):
        if e <= b:
            continue
        ty, tx = divmod(tile, gx)
        ys, xs = np.arange(ty * 16, min(H, ty * 16 + 16)), np.arange(tx * 16, min(W, tx * 16 + 16))
        pix = (ys[:, None] * W + xs[None, :]).reshape(-1)
        where = np.full(N, -1, np.int64)
        where[ref["sorted_ids"][b:e].astype(np.int64)] = np.arange(e - b)
        sub = ids[pix]
        pos[pix] = np.where(sub >= 0, where[np.clip(sub, 0, None)], -1)
    return pos


def chunk_statistics(case, K):
    """What makes a case a test of the reloads: dict(past_first_chunk = pixels that composite an entry of list position >= 256,
    out_of_chunk_order = pixels that composite a hit of an earlier chunk after a hit of a later one, max_hits, full_buffers = pixels
    with more than K hits, terminated_pending = rays that fell below min_transmittance between entry 256 and the end of the list
    with hits still pending in their buffer, terminated_in_drain = rays that did so while the drain composited, not_terminated)."""
    kb = kbuffer(case, K)
    pos = list_positions(case, kb)
    chunk = np.where(pos >= 0, pos // K_STAGE, -1)
    run_max = np.maximum.accumulate(chunk, axis=1)
    cnt = kb["order_count"]
    valid = np.arange(pos.shape[1])[None, :] < cnt[:, None]
    T_final = 1.0 - kb["rgba"].reshape(-1, 4)[:, 3]
    terminated = T_final < case["params"]().min_transmittance
    walk = kb["walk"]
    W, H, gx = case["W"], case["H"], (case["W"] + 15) // 16
    py, px = np.divmod(np.arange(W * H), W)
    length_of_pixel = cc.list_lengths(case["ref"])[(py // 16) * gx + px // 16]
    return dict(past_first_chunk=int(((pos >= K_STAGE) & valid).any(1).sum()),
                out_of_chunk_order=int(((chunk < run_max) & valid).any(1).sum()),
                max_hits=int(cnt.max()), full_buffers=int((cnt > K).sum()),
                terminated_pending=int((terminated & (walk[:, 0] > K_STAGE) & (walk[:, 0] < length_of_pixel) & (walk[:, 1] > 0)).sum()),
                terminated_in_drain=int((terminated & (walk[:, 0] == length_of_pixel) & (walk[:, 1] > 0)).sum()),
                terminated=int(terminated.sum()), not_terminated=int((~terminated & (cnt > 0)).sum()),
                list_lengths=cc.list_lengths(case["ref"]).tolist())


def adjacent_clone_pixels(case, K):
    """Pixels on which at least two clones of one group are composited next to each other, as a boolean [P]."""
    kb = kbuffer(case, K)
    ids = kb["order_ids"]
    g = np.where(ids >= 0, case["group"][np.clip(ids, 0, None)], -1)
    return ((g[:, 1:] == g[:, :-1]) & (g[:, 1:] >= 0)).any(1)
