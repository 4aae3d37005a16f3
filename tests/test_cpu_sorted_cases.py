"""The cases of tests/sorted_cases.py on the CPU oracle alone: every case is built, it reaches the edge of the sorted kernels it is
named for (reloads of the staged list with the k-buffer carried across, a termination with hits pending, an order decided by the
insertion rule), and the oracle's own two-evaluation band stays inside the model AND inside the caps the GPU helpers enforce
(outliers <= 0.5 % of the pixels, rows needing their budget <= 2 % of the non-zero rows).  tests/test_gpu_sorted_variant.py runs
the same cases on the device."""
import importlib

import numpy as np
import pytest

from tests import sorted_cases as sc
from tests.common import COLOUR_TOL, FLIP_MARGIN_BOUND, ROW_FLIP_BOUND
from tests.test_cpu_oracle import _band_pixels, _band_rows

oracle = importlib.import_module("oracle.oracle")


@pytest.mark.parametrize("length", [255, 256, 257, 513, 1025])
def test_single_tile_lists_reach_the_reloads(length):
    case = sc.single_tile(length)
    st = {K: sc.chunk_statistics(case, K) for K in (1, 16)}
    print(f"[sorted case {case['name']}] {st}")
    assert st[16]["list_lengths"] == [length]
    past = {255: 0, 256: 0, 257: 1, 513: 76, 1025: 108}[length]
    for K in (1, 16):
        assert st[K]["past_first_chunk"] == past, "the count of pixels that composite an entry past the first staging moved"
        assert st[K]["terminated"] == 0                       # every ray walks the whole list: all reloads happen
    assert st[1]["out_of_chunk_order"] == 0                   # K = 1 composites in list order
    if length in (513, 1025):
        assert st[16]["out_of_chunk_order"] >= 5              # a hit of an earlier chunk composited after a hit of a later one
        assert st[16]["max_hits"] > sc.K_MAX and st[16]["full_buffers"] >= 10      # the buffer runs full
    else:
        assert st[16]["out_of_chunk_order"] == 0


def test_terminating_deep_list_ends_rays_with_hits_pending():
    case = sc.terminating_deep_list()
    for K in (1, 8, 16):
        st = sc.chunk_statistics(case, K)
        print(f"[sorted case {case['name']} K={K}] {st}")
        assert st["list_lengths"][0] > 4 * sc.K_STAGE
        assert st["terminated_pending"] >= 16 and st["not_terminated"] >= 16


def test_geometry_clones_are_ordered_by_the_insertion_rule():
    a, b = sc.geometry_clones(False), sc.geometry_clones(True)
    assert np.array_equal(a["ref"]["depth"][a["group"] >= 0], b["ref"]["depth"][b["group"] >= 0])
    for g in range(len(sc.CLONE_GROUPS)):
        rows = a["d12"][a["group"] == g]
        assert len(rows) == sc.CLONE_GROUPS[g]
        assert (rows[:, 0:3].view(np.uint32) == rows[0, 0:3].view(np.uint32)).all() and (rows[:, 4:11].view(np.uint32) == rows[0, 4:11].view(np.uint32)).all()
        assert len(np.unique(rows[:, 3])) == len(rows)
    for K in (1, 2, 4, 16):
        ka, kb = sc.kbuffer(a, K), sc.kbuffer(b, K)
        adj = sc.adjacent_clone_pixels(a, K)
        diff = np.abs(ka["rgba"] - kb["rgba"]).max(-1).reshape(-1)
        both = adj & (diff > 10 * COLOUR_TOL)
        order_prone = int((ka["margins"].reshape(-1, 3)[:, 2] < FLIP_MARGIN_BOUND).sum())
        print(f"[sorted case geometry_clones K={K}] clones adjacent on {int(adj.sum())} pixels, reversing them moves {int(both.sum())} of those by "
              f"more than 10 x COLOUR_TOL (largest {float(diff.max()):.3f}); {order_prone} pixels have an order decision within the bound")
        assert both.sum() >= 64
        # bit-equal hit distances earn no allowance: the clones' comparisons have no margin, so these pixels are held to COLOUR_TOL
        calm = ka["margins"].reshape(-1, 3).min(-1) >= FLIP_MARGIN_BOUND
        assert (both & calm).sum() >= 64


def test_order_pairs_make_order_decisions_common():
    case = sc.order_pairs()
    d12 = case["d12"]
    for i, j in case["pairs"]:
        assert np.array_equal(d12[i, [0, 1, 4, 5, 6, 7, 8, 9, 10]], d12[j, [0, 1, 4, 5, 6, 7, 8, 9, 10]]) and d12[i, 2] < d12[j, 2]
        assert abs(int(d12[i, 2:3].view(np.int32)[0]) - int(d12[j, 2:3].view(np.int32)[0])) <= 4
    om = sc.kbuffer(case, 16)["margins"].reshape(-1, 3)[:, 2]
    print(f"[sorted case order_pairs] {int((om < FLIP_MARGIN_BOUND).sum())} of {om.size} pixels have an order decision within the bound")
    assert (om < FLIP_MARGIN_BOUND).sum() >= 500


def test_rays_from_a_centre_plane_meet_an_exactly_zero_hit_distance():
    case = sc.rays_from_a_centre_plane()
    cam = case["view"]["oracle_cam"]
    assert case["ref"]["tiles_count"][0] == 16                  # Gaussian 0 is listed on every tile
    passed = 0
    for py in range(2, 64, 4):
        for px in range(2, 64, 4):
            dbg = oracle.debug_ray(cam, case["ref"], px, py)
            row = dbg[dbg[:, 0] == 0]
            passed += int(len(row) and row[0, 5] == 1 and row[0, 3] > 0.05)
    for K in (1, 16):
        kb = sc.kbuffer(case, K)
        assert not (kb["order_ids"] == 0).any(), "Gaussian 0 is composited: its hit distance is not exactly zero"
        assert kb["order_count"].max() >= 8                      # the rest of the scene is hit as usual
        calm = int((kb["margins"].min(-1) >= FLIP_MARGIN_BOUND).sum())
        print(f"[sorted case rays_from_a_centre_plane K={K}] Gaussian 0 passes the response and alpha tests with alpha > 0.05 on {passed} of 256 "
              f"probed pixels and is composited on none; {calm} of 4096 pixels have no decision within the bound")
        assert passed >= 64 and calm >= 0.95 * 4096


BAND_CASES = {
    **{f"single_tile_{n}": (lambda n=n: sc.single_tile(n)) for n in (255, 256, 257, 513, 1025)},
    "terminating_deep_list": sc.terminating_deep_list,
    "geometry_clones": sc.geometry_clones,
    "rays_from_a_centre_plane": sc.rays_from_a_centre_plane,
    **{name: (lambda name=name: sc.existing(name)) for name in sc.EXISTING},
    "c1_negative_colours": lambda: sc.existing("c1_pinhole_128", negative_colours=True),
}


@pytest.mark.parametrize("name", list(BAND_CASES))
def test_the_oracle_alone_stays_within_the_model_and_the_caps(name):
    """Variant 0 against variants 1 and 2 of the k-buffer oracle on every case the GPU test uses, at K = 1, 8 and 16: margins, pixel
    budget, row budget (test_cpu_oracle's statements, K_BAND to spare) and the helpers' caps.  A case that does not stay inside is
    replaced by another scene; the cap is not raised."""
    case = BAND_CASES[name]()
    cam, W, H, view = case["view"]["oracle_cam"], case["W"], case["H"], case["view"]
    rng = np.random.default_rng(11)
    rg = rng.normal(size=(H, W, 4)).astype(np.float32)
    dg = (0.1 * rng.normal(size=(H, W, 1))).astype(np.float32)
    for K in (1, 8, 16):
        RA = oracle.kbuffer_backward(cam, case["ref"], K, rg, dg, flip_bound=ROW_FLIP_BOUND)
        margins = RA["ref"]["margins"].min(-1)
        report = {}
        for v in (1, 2):
            with oracle.variant(v):
                B = oracle.forward(cam, W, H, case["d12"], case["sph"], view["ro"], view["rd"])
                RB = oracle.kbuffer_backward(cam, B, K, rg, dg)
            rep = _band_pixels((name, K, v), RA["ref"], RB["ref"], margins, RA["ref"]["pixel_budget"])
            need = _band_rows(rep, (name, K, v), RA["dens_g"], RB["dens_g"], RA["sph_g"], RB["sph_g"], RA["budget"])
            assert need <= 0.02, (name, K, v, need)
            rep["rows_needing_budget_share"] = round(need, 4)
            report[v] = rep
        print(f"[sorted case band {name} K={K}] prone pixels {int((margins < FLIP_MARGIN_BOUND).sum())} of {margins.size}: {report}")
