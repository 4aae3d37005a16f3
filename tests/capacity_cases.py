"""Scenes built to sit on the two on-chip capacities of the forward path, shared by tests/test_cpu_capacity_cases.py (the cases'
preconditions, on the CPU oracle alone) and tests/test_gpu_capacity_edges.py (the same cases on the device):

  * the tile window of the grouped binning (gut_project.hip: tile_window): a workgroup of 256 consecutive Gaussians counts its
    entries in kBinWindow = 1536 LDS bins over the union box of its small footprints (tile boxes of <= kSerialTiles = 12 tiles);
    a larger union, or no small footprint at all, leaves no window and every entry takes its own global atomic;
  * the depth cache of the lazy per-tile order (gut_render_common.h: lazy_select): the first kLazyCache = 4096 depth words of a
    tile's slice sit in LDS, the rest is streamed in every pass; selections take kLazyBatch = 512 entries; a radix bin of <= 64
    members ends the passes, a larger one at one depth is selected by id.

Every builder returns a case: the activated scene rows exactly as both the oracle and the device get them (`d12` [N,12], `sph`
[N,48]: no model, no activation in between, so the CPU preconditions hold bit for bit on the device), the view, the oracle's
forward result and a `check` that asserts the case's preconditions from the oracle's buffers alone.  The constants below restate
the kernels' so that a case says which limit it sits on; the kernels are not read."""
import functools
import importlib

import numpy as np

from tests.common import cams, make_view, scenes

oracle = importlib.import_module("oracle.oracle")

K_WORKGROUP = 256      # Gaussians per workgroup of K1 / k_expand_grouped
K_SERIAL_TILES = 12    # a "small" footprint's tile box has at most this many tiles
K_BIN_WINDOW = 1536    # LDS bins of a workgroup's tile window
K_LAZY_CACHE = 4096    # depth words of a tile's slice kept in LDS by lazy_select
K_LAZY_BATCH = 512     # entries ordered per selection
K_SHORT_BIN = 64       # a radix bin of at most this many members ends the digit passes


# ---- the kernels' tile box, restated -------------------------------------------------------------------------------------------
def _clamp_tile(v, grid):
    return np.where(~(v > 0), 0, np.where(v >= np.float32(grid), grid, v.astype(np.int64))).astype(np.int64)


def tile_boxes(ref, W, H):
    """tile_bbox of every row in float32 numpy from the oracle's proj_pos / extent (bit-identical to the device's):
    x0, y0 = floor((p - 0.5 - e) / 16), x1, y1 = ceil((p - 0.5 + e) / 16), clamped to the grid; x1 / y1 exclusive.
    Returns dict(x0, y0, x1, y1, area, active); rows with extent <= 1e-6 are culled (inactive, area 0)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    p, e = ref["proj_pos"].astype(np.float32), ref["extent"].astype(np.float32)
    half, ts = np.float32(0.5), np.float32(16.0)
    with np.errstate(invalid="ignore"):
        x0 = _clamp_tile(np.floor((p[:, 0] - half - e[:, 0]) / ts), gx)
        y0 = _clamp_tile(np.floor((p[:, 1] - half - e[:, 1]) / ts), gy)
        x1 = _clamp_tile(np.ceil((p[:, 0] - half + e[:, 0]) / ts), gx)
        y1 = _clamp_tile(np.ceil((p[:, 1] - half + e[:, 1]) / ts), gy)
    active = ~(e[:, 0] <= np.float32(1e-6))
    area = np.where(active, (x1 - x0) * (y1 - y0), 0)
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, area=area, active=active)


def workgroup_windows(boxes):
    """Per workgroup of 256 consecutive rows what tile_window decides: dict(rows, active, small, union (tiles of the union box of
    the small footprints, 0 without one), window ((x0, y0, w, h) or None))."""
    n = len(boxes["area"])
    out = []
    for k in range(0, n, K_WORKGROUP):
        sl = slice(k, min(n, k + K_WORKGROUP))
        area, act = boxes["area"][sl], boxes["active"][sl]
        small = act & (area > 0) & (area <= K_SERIAL_TILES)
        union, window = 0, None
        if small.any():
            x0, y0 = int(boxes["x0"][sl][small].min()), int(boxes["y0"][sl][small].min())
            w, h = int(boxes["x1"][sl][small].max()) - x0, int(boxes["y1"][sl][small].max()) - y0
            union = w * h
            if union <= K_BIN_WINDOW:
                window = (x0, y0, w, h)
        out.append(dict(rows=(sl.start, sl.stop), active=int(act.sum()), small=int(small.sum()), large=int((area > K_SERIAL_TILES).sum()),
                        union=union, window=window))
    return out


def entry_kinds(ref, boxes, wins, W):
    """The list entries of every workgroup (the oracle's unsorted (tile | depth) keys, row by row) by footprint size and by
    whether their tile lies in the workgroup's window: per workgroup dict(small_in, small_out, large_in, large_out)."""
    gx = (W + 15) // 16
    tile = (ref["unsorted_keys"] >> np.uint64(32)).astype(np.int64)
    end = ref["tiles_offset"].astype(np.int64)
    start = end - ref["tiles_count"].astype(np.int64)
    out = []
    for wg in wins:
        kinds = dict(small_in=0, small_out=0, large_in=0, large_out=0)
        for i in range(*wg["rows"]):
            t = tile[start[i]:end[i]]
            if not t.size:
                continue
            inside = np.zeros(t.size, bool)
            if wg["window"] is not None:
                x0, y0, w, h = wg["window"]
                tx, ty = t % gx, t // gx
                inside = (tx >= x0) & (tx < x0 + w) & (ty >= y0) & (ty < y0 + h)
            size = "small" if boxes["area"][i] <= K_SERIAL_TILES else "large"
            kinds[size + "_in"] += int(inside.sum())
            kinds[size + "_out"] += int((~inside).sum())
        out.append(kinds)
    return out


def list_lengths(ref):
    return ref["tile_ranges"][:, 1].astype(np.int64) - ref["tile_ranges"][:, 0].astype(np.int64)


def fully_walked(ref):
    """Every tile's list is walked to its end by the oracle (no tile terminates early)."""
    return np.array_equal(ref["tile_traversed_fwd"].astype(np.int64), list_lengths(ref))


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _params(tile_culling):
    prm = oracle.default_params()
    prm.tile_culling = 1 if tile_culling else 0
    return prm


def _case(name, sc, W, H, fx, tile_culling, check, eye_z=-4.0):
    view = make_view("pinhole", W, H, cams.look_at_c2w((0, 0, eye_z), (0, 0, 0)), fx=fx)
    d12 = np.ascontiguousarray(scenes.pack_density(sc))
    sph = np.ascontiguousarray(sc["features"].astype(np.float32))
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3, params=_params(tile_culling))
    case = dict(name=name, W=W, H=H, view=view, d12=d12, sph=sph, ref=ref, tile_culling=bool(tile_culling),
                conf={"splat": {"tile_based_culling": bool(tile_culling)}}, check=check, info={})
    case["params"] = lambda: _params(tile_culling)
    check(case)
    return case


def check_preconditions(case):
    """Asserts what makes the case a test of its limit, from the oracle's buffers; fills and returns case["info"]."""
    case["check"](case)
    return case["info"]


def _pixel_scene(n, seed, W, H, fx, uv, depth, scale, density):
    """n Gaussians whose centres project to the pixels uv [n,2] at the given depths from the camera at (0, 0, -4) looking down +z
    (world axes = camera axes); rotations and colours from scene_c1, mildly anisotropic scales around `scale`."""
    rng = np.random.default_rng(seed + 1000)
    sc = scenes.scene_c1(n, seed)
    uv, depth = np.asarray(uv, np.float64), np.asarray(depth, np.float64)
    sc["positions"] = np.stack([(uv[:, 0] - W / 2) / fx * depth, (uv[:, 1] - H / 2) / fx * depth, depth - 4.0], 1).astype(np.float32)
    sc["scale"] = (np.asarray(scale, np.float64)[:, None] * rng.uniform(0.75, 1.3, size=(n, 3))).astype(np.float32)
    sc["density"] = np.asarray(density, np.float32).reshape(n, 1)
    return sc


def _window_report(case):
    ref, W, H = case["ref"], case["W"], case["H"]
    boxes = tile_boxes(ref, W, H)
    wins = workgroup_windows(boxes)
    kinds = entry_kinds(ref, boxes, wins, W)
    case["info"].update(boxes=boxes, windows=wins, kinds=kinds, grid=((W + 15) // 16, (H + 15) // 16),
                        window_areas=[w["union"] for w in wins], traversal=int(ref["tile_traversed_fwd"].sum()),
                        longest_list=int(list_lengths(ref).max()))
    assert ref["M"] > 0 and fully_walked(ref), "the window cases compare whole lists: no tile may terminate early"
    return boxes, wins, kinds


def window_grid(width_tiles, tile_culling):
    """A1 (48 x 32 tiles = kBinWindow exactly) / A2 (49 x 32 = 1568 tiles): rows 0 and 1 are small Gaussians in opposite corner
    tiles, so the union box of workgroup 0's small footprints is the whole grid — the largest window there is, or one tile column
    too many for one.  298 more rows of all sizes are scattered over the image; rows 256 ... 299 form a second workgroup, which has a
    window in both cases (the decision is per workgroup)."""
    W, H, n = 16 * width_tiles, 512, 300
    rng = np.random.default_rng(41)
    uv = np.stack([rng.uniform(4, W - 4, n), rng.uniform(4, H - 4, n)], 1)
    scale = np.exp(rng.uniform(np.log(0.004), np.log(0.07), n))
    uv[0], uv[1] = (8.0, 8.0), (W - 8.0, H - 8.0)
    scale[:2] = 0.005
    # workgroup 1: small footprints only, in the left half of the image
    uv[256:, 0] = rng.uniform(20, W / 2 - 40, n - 256)
    scale[256:] = 0.005
    sc = _pixel_scene(n, 41, W, H, float(W), uv, rng.uniform(3.5, 4.5, n), scale, rng.uniform(0.02, 0.12, n))

    def check(case):
        boxes, wins, kinds = _window_report(case)
        gx, gy = case["info"]["grid"]
        assert (gx, gy) == (width_tiles, 32) and len(wins) == 2
        for r, corner in ((0, (0, 0, 1, 1)), (1, (gx - 1, gy - 1, gx, gy))):
            assert (boxes["x0"][r], boxes["y0"][r], boxes["x1"][r], boxes["y1"][r]) == corner, "a corner Gaussian left its corner tile"
        assert wins[0]["union"] == gx * gy and wins[0]["large"] > 0 and wins[0]["small"] > 100
        if gx * gy <= K_BIN_WINDOW:
            assert wins[0]["union"] == K_BIN_WINDOW and wins[0]["window"] == (0, 0, gx, gy)      # the largest window there is
            assert kinds[0]["small_in"] > 0 and kinds[0]["large_in"] > 0 and kinds[0]["small_out"] + kinds[0]["large_out"] == 0
        else:
            assert wins[0]["union"] > K_BIN_WINDOW and wins[0]["window"] is None                   # small footprints, yet no window
            assert kinds[0]["small_out"] > 0 and kinds[0]["large_out"] > 0 and kinds[0]["small_in"] + kinds[0]["large_in"] == 0
        assert wins[1]["window"] is not None and 0 < wins[1]["union"] < gx * gy and kinds[1]["small_in"] > 0

    return _case(f"window_grid_{width_tiles}x32", sc, W, H, float(W), tile_culling, check)


def no_small_footprint(tile_culling):
    """A3: all 256 rows of workgroup 0 are visible with tile boxes of more than kSerialTiles tiles (no small footprint: no window),
    workgroup 1 (rows 256 ... 399) is all small footprints (a window)."""
    W, H, n = 320, 192, 400
    rng = np.random.default_rng(43)
    uv = np.stack([rng.uniform(30, W - 30, n), rng.uniform(30, H - 30, n)], 1)
    scale = np.where(np.arange(n) < 256, np.exp(rng.uniform(np.log(0.25), np.log(0.5), n)), 0.012)
    sc = _pixel_scene(n, 43, W, H, float(W), uv, rng.uniform(3.5, 4.5, n), scale, rng.uniform(0.02, 0.05, n))

    def check(case):
        boxes, wins, kinds = _window_report(case)
        assert len(wins) == 2
        assert wins[0]["active"] == 256 and wins[0]["large"] == 256 and wins[0]["small"] == 0 and wins[0]["window"] is None
        assert kinds[0]["large_out"] > 256 and kinds[0]["large_in"] == 0
        assert wins[1]["active"] == n - 256 and wins[1]["small"] == n - 256 and wins[1]["window"] is not None and kinds[1]["small_in"] > 0

    return _case("no_small_footprint", sc, W, H, float(W), tile_culling, check)


def partial_last_workgroup(n, tile_culling):
    """A4: N = 257 / 300 — the last workgroup has 1 / 44 rows, the rest of its lanes are beyond N.  Every seventh row lies behind
    the camera (culled: extent 0) inside workgroups that have a window."""
    assert n > K_WORKGROUP and n % K_WORKGROUP
    W, H = 208, 112
    rng = np.random.default_rng(47)
    uv = np.stack([rng.uniform(4, W - 4, n), rng.uniform(4, H - 4, n)], 1)
    scale = np.exp(rng.uniform(np.log(0.01), np.log(0.5), n))
    scale[K_WORKGROUP:] = 0.012                     # the last workgroup's rows are small: it has a window
    depth = rng.uniform(3.5, 4.5, n)
    behind = (np.arange(n) % 7) == 3
    behind[K_WORKGROUP] = False
    depth[behind] = -2.0
    sc = _pixel_scene(n, 47, W, H, float(W), uv, depth, scale, rng.uniform(0.02, 0.08, n))

    def check(case):
        boxes, wins, kinds = _window_report(case)
        assert len(wins) == 2 and wins[1]["rows"] == (K_WORKGROUP, n)
        assert np.array_equal(~boxes["active"], behind) and (case["ref"]["tiles_count"][behind] == 0).all()
        for k, wg in enumerate(wins):
            rows = slice(*wg["rows"])
            assert wg["window"] is not None and kinds[k]["small_in"] > 0
            assert wg["active"] + int(behind[rows].sum()) == rows.stop - rows.start
        assert behind[:K_WORKGROUP].sum() > 30 and (n == K_WORKGROUP + 1 or behind[K_WORKGROUP:].sum() > 3)
        assert wins[0]["large"] > 0 and kinds[0]["large_in"] > 0

    return _case(f"partial_last_workgroup_{n}", sc, W, H, float(W), tile_culling, check)


def large_footprints_across_the_window(tile_culling):
    """A5: one workgroup whose 200 small footprints cluster in the middle of a 20 x 12 grid (the window), and 56 large footprints
    centred on the cluster's rim: their entries fall partly inside the window (LDS bins) and partly outside (global atomics)."""
    W, H, n = 320, 192, 256
    rng = np.random.default_rng(53)
    uv = np.stack([rng.uniform(112, 208, n), rng.uniform(72, 120, n)], 1)
    scale = np.full(n, 0.012)
    big = rng.permutation(n)[:56]
    ang = rng.uniform(0, 2 * np.pi, big.size)
    uv[big] = np.stack([160 + 60 * np.cos(ang), 96 + 36 * np.sin(ang)], 1)
    scale[big] = np.exp(rng.uniform(np.log(0.2), np.log(0.45), big.size))
    sc = _pixel_scene(n, 53, W, H, float(W), uv, rng.uniform(3.5, 4.5, n), scale, rng.uniform(0.02, 0.06, n))

    def check(case):
        boxes, wins, kinds = _window_report(case)
        gx, gy = case["info"]["grid"]
        assert len(wins) == 1 and wins[0]["window"] is not None and wins[0]["union"] < gx * gy // 2
        assert wins[0]["small"] == n - big.size and wins[0]["large"] == big.size
        assert kinds[0]["large_in"] > 0 and kinds[0]["large_out"] > 0 and kinds[0]["small_in"] > 0 and kinds[0]["small_out"] == 0

    return _case("large_footprints_across_the_window", sc, W, H, float(W), tile_culling, check)


WINDOW_CASES = {
    "grid_1536": lambda culling: window_grid(48, culling),
    "grid_1568": lambda culling: window_grid(49, culling),
    "no_small_footprint": no_small_footprint,
    "n_257": lambda culling: partial_last_workgroup(257, culling),
    "n_300": lambda culling: partial_last_workgroup(300, culling),
    "large_across_window": large_footprints_across_the_window,
}


# ---- deep lists ----------------------------------------------------------------------------------------------------------------
DEEP_LENGTHS = (511, 512, 513, 1024, 1025, 4095, 4096, 4097, 4608, 5121, 8193)


def _faint_scene(n, seed, faint, opaque_share=0.02, opaque=0.3):
    sc = scenes.scene_c1(n, seed)
    rng = np.random.default_rng(seed + 77)
    sc["density"] = np.where(rng.random((n, 1)) < opaque_share, opaque, faint).astype(np.float32)
    return sc


def _subset(sc, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in sc.items()}


@functools.lru_cache(maxsize=None)
def _single_tile_base():
    """scene_c1(16000) seen from z = -4 through one 16 x 16 tile, density 0.03 (0.3 for 2 % of the rows): the scene, the ids of the
    tile's list in depth order."""
    sc = _faint_scene(16000, 61, 0.03)
    case = _case("single_tile_base", sc, 16, 16, 16.0, True, lambda c: None)
    ref = case["ref"]
    assert ref["tile_ranges"].shape[0] == 1 and fully_walked(ref)
    return sc, ref["sorted_ids"].astype(np.int64).copy()


def _check_deep(case, length=None, min_length=None):
    ref = case["ref"]
    lens = list_lengths(ref)
    if length is not None:
        assert lens.tolist() == [length], f"the list has {lens.tolist()} entries, not {length}"
    if min_length is not None:
        assert lens.min() > min_length
    # the oracle walks every list to its end: entries beyond the depth cache are ordered by a later selection, not skipped
    assert fully_walked(ref), (ref["tile_traversed_fwd"], lens)
    case["info"].update(list_lengths=lens.tolist(), traversal=ref["tile_traversed_fwd"].astype(np.int64).tolist(),
                        selections=[int(-(-l // K_LAZY_BATCH)) for l in lens], beyond_cache=[int(max(0, l - K_LAZY_CACHE)) for l in lens],
                        max_hits=int(ref["hits"].max()))


def single_tile_list(length):
    """B: one tile whose list has exactly `length` entries and is walked to its end.  The exact length comes from deleting listed
    Gaussians (projection is per Gaussian: the others stay listed; fewer entries only leave the rays more transparent); the
    storage order is shuffled with a fixed seed, so the slice's first kLazyCache words are no depth prefix."""
    sc, listed = _single_tile_base()
    assert len(listed) >= length
    rng = np.random.default_rng(1000 + length)
    drop = rng.permutation(listed)[:len(listed) - length]
    keep = np.setdiff1d(np.arange(len(sc["positions"])), drop)
    sub = _subset(sc, rng.permutation(keep))
    return _case(f"single_tile_{length}", sub, 16, 16, 16.0, True, lambda c: _check_deep(c, length=length))


def four_deep_tiles():
    """C: 32 x 32 pixels, four tiles whose lists all exceed the depth cache and are all walked to their ends: the per-tile cursors
    and slices of several deep tiles filled at once by the grouped expansion."""
    sc = _faint_scene(20000, 67, 0.02)
    return _case("four_deep_tiles", sc, 32, 32, 32.0, True, lambda c: _check_deep(c, min_length=K_LAZY_CACHE + K_LAZY_BATCH))


EARLY_LENGTH, EARLY_FIRST_OPAQUE = 8193, 4700


def deep_list_ending_early():
    """E: the single-tile list of 8193 entries whose entries of depth rank >= 4700 are opaque (density 0.99) and cover the tile
    (scales 1.5: every pixel of the tile within 1.5 sigma).  Every ray walks the 4700 faint entries in front — nine selections, the
    last beyond the depth cache — and ends within a few dozen entries behind them: the walk stops inside the tenth selection, more
    than six selections before the list's end.  What lies behind is never ordered by the lazy order: ordered_ids keeps its padding
    there, tile_traversed_fwd < the list length bounds the backward and every walk (`range.y = range.x + min(..., tile_walked)`),
    and the chunk the walk ends in is cut by s_first_invalid / the depth at which the last ray ended."""
    sc, listed = _single_tile_base()
    rng = np.random.default_rng(1000 + EARLY_LENGTH + 1)
    drop = rng.permutation(listed)[:len(listed) - EARLY_LENGTH]
    order = listed[~np.isin(listed, drop)]                                   # the kept list, in depth order
    sc = {k: v.copy() for k, v in sc.items()}
    opaque = order[EARLY_FIRST_OPAQUE:]
    sc["density"][opaque] = 0.99
    sc["scale"][opaque] = 1.5
    keep = np.setdiff1d(np.arange(len(sc["positions"])), drop)
    sub = _subset(sc, rng.permutation(keep))

    def check(case):
        ref = case["ref"]
        lens = list_lengths(ref)
        assert lens.tolist() == [EARLY_LENGTH], f"the list has {lens.tolist()} entries, not {EARLY_LENGTH}"
        assert EARLY_LENGTH > K_LAZY_CACHE + 2 * K_LAZY_BATCH
        walked = int(ref["tile_traversed_fwd"][0])
        # at least one selection beyond the cache is made, at least one is never made
        assert K_LAZY_CACHE + K_LAZY_BATCH < walked < EARLY_LENGTH - K_LAZY_BATCH, walked
        assert walked > EARLY_FIRST_OPAQUE, "some ray must reach the opaque entries"
        # no pixel is still alive at the end: every ray's last accepted entry leaves T below min_transmittance
        prm = case["params"]()
        cam = case["view"]["oracle_cam"]
        last_t, ended_at = [], []
        for py in range(case["H"]):
            for px in range(case["W"]):
                e = oracle.debug_ray(cam, ref, px, py, params=prm, max_entries=EARLY_LENGTH)
                acc = e[e[:, 5] != 0]
                assert len(acc), (px, py)
                last_t.append(float(acc[-1, 6]))
                ended_at.append(len(e))
        assert max(last_t) < prm.min_transmittance, max(last_t)
        assert max(ended_at) == walked
        case["info"].update(list_lengths=lens.tolist(), traversal=[walked], selections_made=int(-(-walked // K_LAZY_BATCH)),
                            selections_never_made=int(-(-EARLY_LENGTH // K_LAZY_BATCH)) - int(-(-walked // K_LAZY_BATCH)),
                            first_ray_ends_at=min(ended_at), max_hits=int(ref["hits"].max()))

    return _case("deep_list_ending_early", sub, 16, 16, 16.0, True, check)


TIE_GROUPS = (700, 65, 64)


def ties_across_the_cache():
    """D: the single-tile list cut to 9000 entries, in which three Gaussians are each replaced by a group of clones (bit-equal depth,
    ordered by particle id): 700 (more than a selection: the group straddles a selection boundary, the next selection starts
    inside it with ties of the last entry taken on both sides of the depth cache), 65 and 64 (one more than, and exactly, what ends
    the digit passes; each group is placed across a selection boundary so that it IS the bin of the selection's last entry).  The
    clones are spread uniformly over the storage order."""
    sc, listed = _single_tile_base()
    rng = np.random.default_rng(71)
    base_len = 9000
    drop = rng.permutation(listed)[:len(listed) - base_len]
    order = listed[~np.isin(listed, drop)]                                   # the kept list, in depth order
    keep = np.setdiff1d(np.arange(len(sc["positions"])), drop)
    # the group of m members that replaces the entry of rank r occupies ranks r + (members added in front) ... + m - 1; choose the
    # parents, front to back, so that a multiple of 512 lies strictly inside every group
    parents, added = [], 0
    for m, boundary, lead in zip(TIE_GROUPS, (None, 13 * K_LAZY_BATCH, 16 * K_LAZY_BATCH), (0, 30, 30)):
        rank = (boundary - lead) if boundary is not None else 4500 + added
        parents.append(int(order[rank - added]))
        added += m - 1
    assert len(set(parents)) == len(parents)
    keep = keep[~np.isin(keep, parents)]
    rows = [_subset(sc, rng.permutation(keep))]
    for m, p in zip(TIE_GROUPS, parents):
        clone = _subset(sc, np.full(m, p))
        clone["density"][:] = 0.03
        rows.append(clone)
    n_base, n_clone = len(keep), sum(TIE_GROUPS)
    n = n_base + n_clone
    # clones at uniformly spaced storage positions (the three groups interleaved), base rows in between
    clone_pos = np.linspace(0, n - 1, n_clone).round().astype(np.int64)
    assert len(np.unique(clone_pos)) == n_clone
    src = np.empty(n, np.int64)
    is_clone = np.zeros(n, bool)
    is_clone[clone_pos] = True
    src[~is_clone] = np.arange(n_base)
    src[is_clone] = n_base + rng.permutation(n_clone)
    allrows = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    final = _subset(allrows, src)
    group_of = np.full(n, -1)
    bounds = np.cumsum((0,) + TIE_GROUPS) + n_base
    for g in range(len(TIE_GROUPS)):
        group_of[(src >= bounds[g]) & (src < bounds[g + 1])] = g

    def check(case):
        ref = case["ref"]
        _check_deep(case, length=base_len - len(TIE_GROUPS) + n_clone)
        depth_bits = ref["depth"].view(np.uint32)
        ids = ref["sorted_ids"].astype(np.int64)
        spans = []
        for g, m in enumerate(TIE_GROUPS):
            members = np.nonzero(group_of == g)[0]
            assert len(members) == m and len(np.unique(depth_bits[members])) == 1, "clones must share their depth bits"
            assert int((depth_bits == depth_bits[members[0]]).sum()) == m, "nothing else may sit at the clones' depth"
            ranks = np.nonzero(np.isin(ids, members))[0]
            assert len(ranks) == m and ranks[-1] - ranks[0] == m - 1                       # one run of the sorted list
            assert np.array_equal(ids[ranks], np.sort(members))                            # ... ordered by particle id
            inside = [q for q in range(ranks[0] + 1, ranks[-1] + 1) if q % K_LAZY_BATCH == 0]
            assert inside, f"no selection boundary inside the group of {m} (ranks {ranks[0]} ... {ranks[-1]})"
            # storage positions on both sides of the depth cache would follow from the uniform spread if the slice kept the
            # storage order; the expansion's order is arbitrary, so this is reported, not asserted
            spans.append((int(ranks[0]), int(ranks[-1])))
        case["info"].update(tie_ranks=spans)

    return _case("ties_across_the_cache", final, 16, 16, 16.0, True, check)
