"""The capacity cases of tests/capacity_cases.py on the CPU oracle alone: every case is built, its preconditions hold (the window
of every workgroup is the one the case is named for, every deep list has its exact length and is walked to its end, the tie
groups lie across selection boundaries), and the float32 restatement of the kernels' tile box that those preconditions rest on
agrees with the oracle's own tile counts.  tests/test_gpu_capacity_edges.py runs the same cases on the device."""
import numpy as np
import pytest

from tests import capacity_cases as cc
from tests import contribution_reference as cr


@pytest.mark.parametrize("name", list(cc.WINDOW_CASES))
def test_tile_box_restatement_matches_the_oracle_counts(name):
    """Without tile-based culling a Gaussian's tile count IS its box area: on every visible row of every window case."""
    case = cc.WINDOW_CASES[name](False)
    boxes = cc.tile_boxes(case["ref"], case["W"], case["H"])
    count = case["ref"]["tiles_count"].astype(np.int64)
    assert (count > 0).sum() > 100
    assert np.array_equal(boxes["area"], count)
    assert np.array_equal(boxes["active"] & (boxes["area"] > 0), count > 0)
    # with culling the box only bounds the count
    culled = cc.WINDOW_CASES[name](True)
    assert np.array_equal(culled["ref"]["extent"], case["ref"]["extent"]) and np.array_equal(culled["ref"]["proj_pos"], case["ref"]["proj_pos"])
    assert (culled["ref"]["tiles_count"].astype(np.int64) <= boxes["area"]).all()


@pytest.mark.parametrize("tile_culling", [True, False])
@pytest.mark.parametrize("name", list(cc.WINDOW_CASES))
def test_window_cases_sit_on_their_limit(name, tile_culling):
    case = cc.WINDOW_CASES[name](tile_culling)
    info = cc.check_preconditions(case)
    print(f"[capacity {case['name']} culling={tile_culling}] grid {info['grid']}, window areas {info['window_areas']}, "
          f"windows {[w['window'] for w in info['windows']]}, entries {info['kinds']}, longest list {info['longest_list']}")
    if name == "grid_1536":
        assert info["window_areas"][0] == cc.K_BIN_WINDOW and info["windows"][0]["window"] is not None
    if name == "grid_1568":
        assert info["window_areas"][0] == cc.K_BIN_WINDOW + 32 and info["windows"][0]["window"] is None


@pytest.mark.parametrize("length", cc.DEEP_LENGTHS)
def test_single_tile_lists_have_their_exact_length(length):
    case = cc.single_tile_list(length)
    info = cc.check_preconditions(case)
    print(f"[capacity {case['name']}] {info}")
    assert info["list_lengths"] == [length] and info["traversal"] == [length]
    assert info["beyond_cache"] == [max(0, length - cc.K_LAZY_CACHE)]
    if length > cc.K_LAZY_CACHE:
        # the walk passes entry 4096 and goes on for at least one more selection's worth of ordered entries
        assert info["selections"][0] > cc.K_LAZY_CACHE // cc.K_LAZY_BATCH


def test_four_deep_tiles():
    case = cc.four_deep_tiles()
    info = cc.check_preconditions(case)
    print(f"[capacity {case['name']}] {info}")
    assert len(info["list_lengths"]) == 4 and min(info["list_lengths"]) > cc.K_LAZY_CACHE


def test_deep_list_ends_early():
    """E: the walk ends beyond the depth cache and more than a selection before the list's end; no ray outlives it."""
    case = cc.deep_list_ending_early()
    info = cc.check_preconditions(case)
    print(f"[capacity {case['name']}] {info}")
    assert info["list_lengths"] == [cc.EARLY_LENGTH]
    assert cc.K_LAZY_CACHE + cc.K_LAZY_BATCH < info["traversal"][0] < cc.EARLY_LENGTH - cc.K_LAZY_BATCH
    assert info["selections_made"] > cc.K_LAZY_CACHE // cc.K_LAZY_BATCH + 1 and info["selections_never_made"] >= 1
    assert not cc.fully_walked(case["ref"])


def test_tie_groups_lie_across_selection_boundaries():
    case = cc.ties_across_the_cache()
    info = cc.check_preconditions(case)
    print(f"[capacity {case['name']}] {info}")
    assert info["list_lengths"][0] > 2 * cc.K_LAZY_CACHE and [b - a + 1 for a, b in info["tie_ranks"]] == list(cc.TIE_GROUPS)


@pytest.mark.parametrize("name", cr.DEEP_CASES)
def test_walk_references_of_the_deep_cases(name):
    """What tests/test_gpu_walk_depth.py rests on, from the references alone: every tile's walk passes the depth cache, rows behind
    the walked prefixes exist and score nothing, the surface references choose an entry on most pixels, and the share of NEAR pixels
    (where another fp32 evaluation may choose another entry) stays under the cap that file allows the case."""
    from tests import surface_reference as sr
    MAX_NEAR = cr.DEEP_MAX_NEAR
    c = cr.case(name)
    ref, k = c["ref"], c["contrib"]
    assert (ref["tile_traversed_fwd"].astype(np.int64) > cc.K_LAZY_CACHE).all()
    assert (~k["walked"]).sum() > 0 and not k["pixels"][~k["walked"]].any() and (k["pixels"] > 0).sum() > cc.K_LAZY_CACHE // 2
    if name == "deep_list_ending_early":
        behind = ref["sorted_ids"][int(ref["tile_traversed_fwd"][0]):]
        assert len(behind) > cc.K_LAZY_BATCH and not k["walked"][behind].any()        # listed, never walked
    s = sr.surface_case(name)
    shares = {}
    for level in sr.LEVELS:
        shares[level] = float(sr.level_planes(name, level)["near"].sum() / s["hit"].sum())
    shares["max_weight"] = float(sr.max_weight_planes(name)["near"].sum() / s["hit"].sum())
    print(f"[deep walk {name}] {int(s['hit'].sum())} pixels with a hit, near shares {shares}")
    assert max(shares.values()) <= MAX_NEAR[name]
    assert (sr.level_planes(name, 0.5)["id"] >= 0).sum() > 0 and (sr.max_weight_planes(name)["id"] >= 0).sum() == s["hit"].sum()
