"""The CPU reference of the per-Gaussian contribution scores (gut_trace_contribution), and the cases both the CPU and
the GPU tests of it use.

`reference(cam, fwd, params)` walks every pixel of an oracle forward with oracle.debug_ray — the entries the pixel walks: id, alpha,
accepted, T after — and forms, for every accepted entry, w = T_before * alpha (T_before: the T after of the pixel's previous accepted
entry, 1 at the start).  Per Gaussian: the sum of w, the largest w and the number of pixels with w > 0.  With the per-pixel decision
margins (oracle.render_margins) it also counts, per Gaussian, its PRONE entries — the entries (accepted or not) it has in pixels
whose smallest margin is below common.FLIP_MARGIN_BOUND, where another valid fp32 evaluation may decide differently — and the
largest w over the pixels that are not prone.

Everything is computed once per case and cached: the tests share it and leave it unchanged."""
import functools
import importlib

import numpy as np

from tests import capacity_cases, off_centre_cases
from tests.common import FLIP_MARGIN_BOUND, FISHEYE_DIST, cams, densified_like_scene, make_view, scenes

oracle = importlib.import_module("oracle.oracle")

CASES = ("pinhole_64x48", "ragged_70x45", "fisheye", "single_tile_1025")
# Further cases, by name, for the tests that go beyond the four above.  `case` and every reference derived from it
# (attribute_reference.attribute_case, attribute_gradient_reference.gradient_case, weighted_contribution_reference.weighted_case,
# surface_reference.surface_case) take these names as well:
#   "<one of CASES>@<plane>"   the case seen through the origin plane `plane` of tests/off_centre_cases.py (rays that do not start at
#                              the sensor position: the un-centred instantiation of k_walk)
#   one of DEEP_CASES          lists beyond the 4096-word depth cache of the lazy order (tests/capacity_cases.py)
#   a name given to `view_case`  any view of a named case's scene
DEEP_CASES = ("single_tile_4097", "four_deep_tiles", "ties_across_the_cache", "deep_list_ending_early")
# The share of a deep case's pixels with a hit that may be NEAR in its surface references (another valid fp32 evaluation may choose
# another entry; tests/surface_reference.py) is a property of the reference alone.  Rays through thousands of faint entries keep a
# wide flip budget: 14.1 % of four_deep_tiles' pixels and 11.4 % of ties_across_the_cache's are near at level 0.1; the other 85 % are
# held to the reference's id exactly.  The two other cases stay under the 5 % of the one-view test.  tests/test_cpu_capacity_cases.py
# asserts the shares, tests/test_gpu_walk_depth.py allows them.
DEEP_MAX_NEAR = {"single_tile_4097": 0.05, "four_deep_tiles": 0.15, "ties_across_the_cache": 0.15, "deep_list_ending_early": 0.05}
_VIEW_CASES = {}


def base_name(name):
    """The case of CASES or DEEP_CASES whose scene the case `name` shows."""
    return _VIEW_CASES[name][0] if name in _VIEW_CASES else name.split("@")[0]


def case_index(name):
    """A small integer per case name, the offset of the seeds the derived references draw their random inputs with: the position in
    CASES for the four cases there and for every other view of their scenes, the positions after them for DEEP_CASES."""
    return (CASES + DEEP_CASES).index(base_name(name))


def reference(cam, fwd, params=None, margins=None):
    """dict(weight_sum [N] f64, max_weight [N] f64, pixels [N] i64, walked [N] bool (some pixel walked the Gaussian), and with
    margins [H,W,2]: prone_entries [N] i64, max_weight_calm [N] f64, prone_pixels)."""
    d12, _, _, _, _, W, H = fwd["_inputs"]
    n = d12.shape[0]
    wsum, wmax, wmax_calm = np.zeros(n), np.zeros(n), np.zeros(n)
    pixels, prone_entries = np.zeros(n, np.int64), np.zeros(n, np.int64)
    walked = np.zeros(n, bool)
    prone_pixels = 0
    longest = int((fwd["tile_ranges"][:, 1].astype(np.int64) - fwd["tile_ranges"][:, 0]).max()) if fwd["M"] else 0
    for py in range(H if fwd["M"] else 0):
        for px in range(W):
            e = oracle.debug_ray(cam, fwd, px, py, params=params, max_entries=max(16, longest))
            if not len(e):
                continue
            ids = e[:, 0].astype(np.int64)
            walked[ids] = True
            prone = margins is not None and float(margins[py, px].min()) < FLIP_MARGIN_BOUND
            if prone:
                prone_pixels += 1
                np.add.at(prone_entries, ids, 1)
            acc = e[:, 5] != 0
            if not acc.any():
                continue
            t_after = e[acc, 6]
            w = np.concatenate([[1.0], t_after[:-1]]) * e[acc, 3]
            a_ids = ids[acc]
            np.add.at(wsum, a_ids, w)
            np.maximum.at(wmax, a_ids, w)
            if not prone:
                np.maximum.at(wmax_calm, a_ids, w)
            np.add.at(pixels, a_ids[w > 0], 1)
    return dict(weight_sum=wsum, max_weight=wmax, pixels=pixels, walked=walked, prone_entries=prone_entries,
                max_weight_calm=wmax_calm, prone_pixels=prone_pixels)


def _scene_case(name, n, seed, view):
    sc = scenes.scene_c1(n, seed)
    d12 = np.ascontiguousarray(scenes.pack_density(sc))
    sph = np.ascontiguousarray(sc["features"].astype(np.float32))
    ref = oracle.forward(view["oracle_cam"], view["W"], view["H"], d12, sph, view["ro"], view["rd"], sh_degree=3)
    return dict(name=name, W=view["W"], H=view["H"], view=view, d12=d12, sph=sph, ref=ref, conf={}, params=lambda: None)


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its oracle forward (`ref`), decision margins, contribution reference (`contrib`) and the oracle backward of
    the cotangent (1, 0, 0, 0): `feat_grad` [N] = d(sum of red)/d(red feature), the second statement of weight_sum, with its flip
    budget and fp32 conditioning."""
    if "@" in name and name not in _VIEW_CASES:
        base, plane = name.split("@")
        view_case(name, base, off_centre_cases.off_centre(_base(base)["view"], plane))
    if name in _VIEW_CASES:           # another view of a named case's scene (view_case)
        base, view = _VIEW_CASES[name]
        b = _base(base)
        c = dict(b, name=name, view=view, info={}, ref=oracle.forward(view["oracle_cam"], b["W"], b["H"], b["d12"], b["sph"], view["ro"], view["rd"],
                                                                      sh_degree=3, params=b["params"]()))
    else:
        c = dict(_base(name))
    return _finish(c)


def view_case(name, base, view):
    """The entry point for a view instead of a case name: registers `name` as the scene of the case `base` seen through `view` (a
    make_view result of the same size, any origin plane) and returns the name; case(name) and the derived references then build it
    like any other, once.  The cases of CASES themselves are not touched."""
    assert base in CASES + DEEP_CASES and name not in CASES + DEEP_CASES
    assert name not in _VIEW_CASES or _VIEW_CASES[name][1] is view, f"{name} is already another view"
    assert (view["W"], view["H"]) == (_base(base)["W"], _base(base)["H"])
    _VIEW_CASES.setdefault(name, (base, view))
    return name


@functools.lru_cache(maxsize=None)
def _base(name):
    """The scene, view and oracle forward of a case of CASES or DEEP_CASES."""
    if name == "pinhole_64x48":     # the case of tests/test_cpu_pose_gradient.py
        c = _scene_case(name, 300, 0, make_view("pinhole", 64, 48, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)), fx=64.0))
    elif name == "ragged_70x45":    # ragged right and bottom tiles, ragged last wave of rows, an orbit pose
        c = _scene_case(name, 333, 0, make_view("pinhole", 70, 45, cams.orbit_c2w(4.0, 37.0, 12.0), fx=70.0))
    elif name == "fisheye":
        c = _scene_case(name, 300, 0, make_view("fisheye", 64, 48, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)),
                                                distortion=FISHEYE_DIST))
    elif name == "single_tile_1025":  # one tile, 1025 entries: five chunks, three lazy-order selections, a last chunk of one entry
        c = dict(capacity_cases.single_tile_list(1025))
    elif name == "single_tile_4097":  # one entry beyond the depth cache: the ninth selection orders one streamed word
        c = dict(capacity_cases.single_tile_list(4097))
    elif name == "four_deep_tiles":
        c = dict(capacity_cases.four_deep_tiles())
    elif name == "ties_across_the_cache":
        c = dict(capacity_cases.ties_across_the_cache())
    elif name == "deep_list_ending_early":
        c = dict(capacity_cases.deep_list_ending_early())
    else:
        raise KeyError(name)
    return c


def _finish(c):
    cam, fwd, W, H = c["view"]["oracle_cam"], c["ref"], c["W"], c["H"]
    prm = c["params"]()
    c["margins"] = oracle.render_margins(cam, fwd, params=prm)
    c["contrib"] = reference(cam, fwd, params=prm, margins=c["margins"])
    cot = np.zeros((H, W, 4), np.float32)
    cot[..., 0] = 1.0
    _, _, feat_g, budget = oracle.backward(cam, fwd, cot, np.zeros((H, W, 1), np.float32), params=prm, flip_bound=FLIP_MARGIN_BOUND)
    c.update(feat_grad=feat_g[:, 0].copy(), flip_budget=budget[:, 4].copy(), fp32_noise=budget[:, 9].copy())
    return c


def planted_scene(n=20000, n_planted=2000, seed=5):
    """densified_like_scene(n) plus n_planted rows no view can see, appended last: half of them small Gaussians at the centre of an
    opaque blob (60 large Gaussians of density 0.999 within 0.15 of the origin, which are part of the scene proper: from every
    direction dozens of them lie in front of the centre and end every ray that reaches it), half with a density below the alpha
    threshold 1 / 255 scattered through the scene (never accepted anywhere).  Returns (scene, planted [N] bool)."""
    rng = np.random.default_rng(seed + 100)
    sc = densified_like_scene(n, seed)
    like = scenes.scene_c1(60 + n_planted, seed + 1)
    blob = {k: v[:60].copy() for k, v in like.items()}
    blob["positions"] = rng.uniform(-0.15, 0.15, (60, 3)).astype(np.float32)
    blob["scale"] = rng.uniform(0.2, 0.3, (60, 3)).astype(np.float32)
    blob["density"] = np.full((60, 1), 0.999, np.float32)
    hidden = {k: v[60:60 + n_planted // 2].copy() for k, v in like.items()}
    hidden["positions"] = rng.uniform(-0.02, 0.02, hidden["positions"].shape).astype(np.float32)
    hidden["scale"] = rng.uniform(0.005, 0.01, hidden["scale"].shape).astype(np.float32)
    hidden["density"] = np.full_like(hidden["density"], 0.9)
    faint = {k: v[60 + n_planted // 2:].copy() for k, v in like.items()}
    faint["positions"] = rng.uniform(-1.0, 1.0, faint["positions"].shape).astype(np.float32)
    faint["density"] = np.full_like(faint["density"], 0.003)
    out = {k: np.ascontiguousarray(np.concatenate([sc[k], blob[k], hidden[k], faint[k]])) for k in sc}
    planted = np.zeros(out["positions"].shape[0], bool)
    planted[-n_planted:] = True
    return out, planted


def planted_views(W=160, H=120):
    return [make_view("pinhole", W, H, cams.orbit_c2w(4.0, 60.0 * i, 10.0 + 8.0 * (i % 3)), fx=1.0 * W) for i in range(6)]
