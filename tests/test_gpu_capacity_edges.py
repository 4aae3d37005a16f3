"""The forward path past its two on-chip capacities, on small cases built to sit on each limit (tests/capacity_cases.py; their
preconditions alone are tests/test_cpu_capacity_cases.py):

  * the tile window of the grouped binning (tile_window, shared by K1's per-tile counts and k_expand_grouped): a window of exactly
    kBinWindow = 1536 tiles, a union box one tile column too large (no window although small footprints exist), a workgroup
    without any small footprint, a partly filled last workgroup with culled rows, large footprints across a window's edge;
  * the depth cache of the lazy per-tile order (lazy_select, K6): single-tile lists of exact lengths around the selection size
    (512), the cache size (4096) and beyond, four deep tiles at once, tie groups of 700 / 65 / 64 clones across selection
    boundaries and across the cache, and a list of 8193 entries whose walk ends at 4727 (case E: the selections behind the last
    ray's end are never made, the backward is bounded by the forward's depth).

Every case is compared with the CPU oracle — tile ranges, counts and offsets bit for bit, the ordered ids over the WHOLE slice of
every tile (cases A - D are walked to the end of every list; case E over its walked prefix, with padding or the oracle's id
behind it), traversal depths, image and hit counts per pixel against the pixel's
own flip budget, every gradient block per row against the row's own budget — and with the full stable sort
(set_lazy_tile_order(False)): outputs and ranges bit-equal, gradients to 1e-5 relative L2.  The inputs are the activated [N,12] /
[N,48] rows themselves (SplatRaster.trace of the Tracer's wrapper), so the oracle's preconditions hold bit for bit on the device."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import capacity_cases as cc
from tests.common import GRAD_BLOCKS, ROW_FLIP_BOUND, check_colour_outliers, check_gradient_rows, rel_l2, to_batch
from tests.test_gpu_parity import _check_ordered_ids

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"
PAD = 0xFFFFFFFF


def _render(case, lazy, rgba_grad):
    """One forward and one backward of the case on a fresh handle; everything the checks read, on the host."""
    tr = gut.Tracer({"render": case["conf"]})
    raster = tr.tracer_wrapper
    raster.set_lazy_tile_order(lazy)
    view = case["view"]
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    cam = (ro, rd, None, sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
    rgba, dist, hits, vis = raster.trace(0, 3, d12, sph, *cam)
    g12, g48 = raster.trace_bwd(0, 3, d12, sph, *cam, rgba, torch.as_tensor(rgba_grad, device=DEV), dist, None)
    u32 = lambda name: raster.debug_buffer(name).cpu().numpy().view(np.uint32)
    return dict(raster=raster, rgba=rgba.cpu().numpy(), dist=dist.cpu().numpy(), hits=hits.cpu().numpy(), g12=g12.cpu().numpy(),
                g48=g48.cpu().numpy(), tile_ranges=u32("tile_ranges").reshape(-1, 2), tile_traversed_fwd=u32("tile_traversed_fwd"),
                stats=raster.stats())


def _check_case(case, walked_to_the_end=True):
    """walked_to_the_end=False (case E): the oracle's walk ends inside the list.  The ordered ids are then compared over the walked
    prefix of every tile; behind it every id is either the oracle's (ordered by the selection the walk ended in) or padding."""
    info = cc.check_preconditions(case)        # again, here: an edited scene must not leave this test testing nothing
    ref, W, H, name = case["ref"], case["W"], case["H"], f"{case['name']}/culling={int(case['tile_culling'])}"
    ocam, prm = case["view"]["oracle_cam"], case["params"]()
    rgba_grad = np.random.default_rng(5).normal(size=(H, W, 4)).astype(np.float32)
    full = _render(case, False, rgba_grad)
    lazy = _render(case, True, rgba_grad)
    raster = lazy["raster"]
    assert lazy["stats"]["num_intersections"] == ref["M"] and full["stats"]["num_intersections"] == ref["M"]

    # the lazy order against the full stable sort (as tests/test_gpu_grouped_binning._compare)
    for key in ("rgba", "dist", "hits", "tile_ranges", "tile_traversed_fwd"):
        assert np.array_equal(full[key], lazy[key]), f"{name}: {key} differs between the lazy order and the full sort"
    for key in ("g12", "g48"):
        assert rel_l2(lazy[key], full[key]) <= 1e-5, f"{name}: {key} lazy vs full sort {rel_l2(lazy[key], full[key])}"

    # integer structure against the oracle: bit-equal
    assert np.array_equal(lazy["tile_ranges"], ref["tile_ranges"]), f"{name}: tile_ranges"
    for key in ("tiles_count", "tiles_offset"):
        assert np.array_equal(raster.debug_buffer(key).cpu().numpy().view(np.uint32), ref[key]), f"{name}: {key}"
    _check_ordered_ids(raster, ref)
    ordered = raster.debug_buffer("ordered_ids").cpu().numpy().view(np.uint32)
    same = ordered == ref["sorted_ids"]
    if not walked_to_the_end:
        behind = np.ones(ordered.size, bool)
        for t, (b, e) in enumerate(ref["tile_ranges"]):
            behind[int(b):int(b) + min(int(ref["tile_traversed_fwd"][t]), int(e) - int(b))] = False
        assert behind.any() and (ordered[behind] == PAD).any(), f"{name}: nothing of the list was left unordered"
        same |= behind & (ordered == PAD)
    bad = np.nonzero(~same)[0]
    where = ""
    if bad.size:
        tile = int(np.searchsorted(ref["tile_ranges"][:, 1], bad[0], side="right"))
        where = f"first at list position {int(bad[0])} = entry {int(bad[0]) - int(ref['tile_ranges'][tile, 0])} of tile {tile}"
    assert not bad.size, f"{name}: {bad.size} of {ordered.size} ordered ids differ from the oracle's sorted list ({int((ordered == PAD).sum())} padding ids), {where}"
    assert np.array_equal(lazy["tile_traversed_fwd"], ref["tile_traversed_fwd"]), f"{name}: traversal depths"
    assert lazy["stats"]["traversed_fwd"] == ref["traversed_fwd"]

    # image and hit counts: every pixel within its own flip budget
    margins, pixel_budget = oracle.render_margins(ocam, ref, params=prm, budget_bound=ROW_FLIP_BOUND)
    pix = check_colour_outliers(lazy["rgba"], lazy["hits"], ref, margins, label=name, budget=pixel_budget)
    calm = margins.min(-1) >= 4.0
    if calm.any():
        d_gpu, d_ref = lazy["dist"].reshape(H, W), ref["dist"].reshape(H, W)
        assert np.abs(d_gpu - d_ref)[calm].max() <= 2e-3 * max(1.0, float(np.abs(d_ref).max()))

    # gradients: every row of every block within its own bound
    dens_g, sph_g, _, budget = oracle.backward(ocam, ref, rgba_grad, np.zeros((H, W, 1), np.float32), params=prm, flip_bound=ROW_FLIP_BOUND)
    rows = {}
    for j, (block, sl) in enumerate(GRAD_BLOCKS):
        rows[block] = check_gradient_rows(lazy["g12"][:, sl], dens_g[:, sl], f"{name}/{block}", budget[:, j], budget[:, 5 + j])
    y = math.sqrt(16 / (4 * math.pi))      # the SH basis norm at degree 3 (tests/common.check_gradients_per_row)
    rows["sh"] = check_gradient_rows(lazy["g48"], sph_g, f"{name}/sh", budget[:, 4] * y, budget[:, 9] * y)
    assert float(np.abs(lazy["g12"][:, 11]).max()) == 0.0
    culled = ref["tiles_count"] == 0
    if culled.any():
        assert float(np.abs(lazy["g12"][culled]).max()) == 0.0 and float(np.abs(lazy["g48"][culled]).max()) == 0.0
    assert lazy["stats"]["traversed_bwd"] == ref["traversed_bwd"]
    worst_row = max(r["worst_row_vs_full_bound"] for r in rows.values())
    size = f"window areas {info['window_areas']}" if "window_areas" in info else f"list lengths {info['list_lengths']}"
    print(f"[capacity {name}] {size}, traversal depth {info['traversal']}, worst pixel / its bound {pix['worst_vs_budget']:.3f}, "
          f"worst row / its bound {worst_row:.3f}")
    return info


@pytest.mark.parametrize("tile_culling", [True, False])
@pytest.mark.parametrize("name", list(cc.WINDOW_CASES))
def test_tile_window_limits(name, tile_culling):
    """A: the window at its largest size (1536 tiles), none although small footprints exist (1568), none for lack of a small
    footprint, a partly inactive last workgroup with culled rows, large footprints inside and outside a window — with and without
    tile-based culling (K1 counts the box without it, the tiles that pass tile_min_power with it)."""
    info = _check_case(cc.WINDOW_CASES[name](tile_culling))
    if name == "grid_1536":
        assert info["window_areas"][0] == cc.K_BIN_WINDOW and info["windows"][0]["window"] is not None
    if name == "grid_1568":
        assert info["window_areas"][0] > cc.K_BIN_WINDOW and info["windows"][0]["window"] is None and info["windows"][0]["small"] > 0


@pytest.mark.parametrize("length", cc.DEEP_LENGTHS)
def test_single_tile_list_of_exact_length(length):
    """B: one tile, one list of exactly `length` entries in shuffled storage order, walked to its end: one selection short of,
    equal to and one past a whole number of selections; one short of, equal to and one past the depth cache; and past it by one
    selection, by two and a bit, by a whole cache."""
    info = _check_case(cc.single_tile_list(length))
    assert info["list_lengths"] == [length] and info["traversal"] == [length]


def test_four_deep_tiles_at_once():
    """C: four tiles, each list longer than the depth cache by more than a selection, all walked to their ends."""
    info = _check_case(cc.four_deep_tiles())
    assert len(info["list_lengths"]) == 4 and min(info["list_lengths"]) > cc.K_LAZY_CACHE + cc.K_LAZY_BATCH


def test_deep_list_that_ends_early():
    """E: 8193 entries on one tile, opaque from depth rank 4700 on: nine selections are walked whole (the ninth beyond the depth
    cache), the tenth is cut short when the last ray ends, seven are never made.  The walked prefix is the oracle's order, what lies
    behind it is ordered or padding, the traversal depth is the oracle's, and the backward — bounded by that depth — gives the
    oracle's rows, under the lazy order and under the full sort."""
    info = _check_case(cc.deep_list_ending_early(), walked_to_the_end=False)
    assert info["list_lengths"] == [cc.EARLY_LENGTH] and cc.K_LAZY_CACHE + cc.K_LAZY_BATCH < info["traversal"][0] < cc.EARLY_LENGTH - cc.K_LAZY_BATCH
    assert info["selections_never_made"] >= 1


def test_depth_ties_across_selections_and_the_cache():
    """D: tie groups of 700, 65 and 64 clones in a list of 9826 entries, each across a selection boundary, the clones spread over
    the storage order (ties with the last entry taken on both sides of the cache; the id select for more than 64 members of one
    depth, the single-wave ranking for exactly 64)."""
    info = _check_case(cc.ties_across_the_cache())
    assert [b - a + 1 for a, b in info["tie_ranks"]] == list(cc.TIE_GROUPS)
