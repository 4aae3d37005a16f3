"""ctypes front-end of the C oracle (oracle/gut_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg, never by the product package.  The per-hit backward is pinned to the reference's
own header (HitUnits below, tests/test_cpu_reference_hits.py); "parity unpinned" for the rest of the
device kernels (the reference ships no fixtures for this path); see gut_oracle.c header.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class OracleParams(C.Structure):
    _fields_ = [
        ("alpha_threshold", C.c_float), ("max_alpha", C.c_float), ("min_kernel_density", C.c_float),
        ("min_transmittance", C.c_float), ("min_sensor_z", C.c_float), ("cov_dilation", C.c_float),
        ("ut_alpha", C.c_float), ("ut_beta", C.c_float), ("ut_kappa", C.c_float), ("ut_margin", C.c_float),
        ("rect_bounding", C.c_int32), ("tight_opacity_bounding", C.c_int32), ("tile_culling", C.c_int32),
        ("global_z_order", C.c_int32),
        ("kernel_degree", C.c_int32), ("rolling_shutter_iterations", C.c_int32), ("enable_hitcounts", C.c_int32),
    ]


class OracleCamera(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("shutter", C.c_int32),
        ("principal_point", C.c_float * 2), ("focal_length", C.c_float * 2),
        ("radial", C.c_float * 6), ("tangential", C.c_float * 2), ("thin_prism", C.c_float * 4),
        ("max_angle", C.c_float), ("pose_start", C.c_float * 7), ("pose_end", C.c_float * 7),
    ]


def build(force=False):
    so = os.path.join(_HERE, "libgut_oracle.so")
    src = os.path.join(_HERE, "gut_oracle.c")
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-B", "libgut_oracle.so"], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.oracle_scan.restype = C.c_uint32
        _LIB.oracle_higher_msb.restype = C.c_uint32
        _LIB.oracle_det_logf.restype = C.c_float
        _LIB.oracle_det_logf.argtypes = [C.c_float]
        _LIB.oracle_det_atan2f.restype = C.c_float
        _LIB.oracle_det_atan2f.argtypes = [C.c_float, C.c_float]
        _LIB.oracle_tile_min_power.restype = C.c_float
        _LIB.oracle_tile_min_power.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    return _LIB


class variant:
    """`with oracle.variant(1): ...` — everything inside evaluates the per-(ray, Gaussian) formulas of the compositing passes in the
    second fp32 form (gut_oracle.c: eval_hit_fused: FMA, pre-scaled rows, one reciprocal, exp2).  Projection and binning are
    unaffected (they carry the bit-exact contract).  Tests only: the measured basis of the GPU tolerances."""

    def __init__(self, v):
        self.v = int(v)

    def __enter__(self):
        self.prev = int(lib().oracle_get_variant())
        lib().oracle_set_variant(C.c_int(self.v))
        return self

    def __exit__(self, *exc):
        lib().oracle_set_variant(C.c_int(self.prev))
        return False


def default_params():
    p = OracleParams()
    lib().oracle_default_params(C.byref(p))
    return p


def make_camera(cam: dict) -> OracleCamera:
    """cam: dict with keys model('pinhole'|'fisheye'), principal_point, focal_length, radial, tangential,
    thin_prism, max_angle, pose_start[7], pose_end[7] (world->sensor t, q xyzw)."""
    c = OracleCamera()
    c.model = 0 if cam["model"] == "pinhole" else 1
    c.shutter = int(cam.get("shutter", 4))
    c.principal_point[:] = [float(v) for v in cam["principal_point"]]
    c.focal_length[:] = [float(v) for v in cam["focal_length"]]
    rad = list(cam.get("radial", [])) + [0.0] * 6
    c.radial[:] = [float(v) for v in rad[:6]]
    c.tangential[:] = [float(v) for v in cam.get("tangential", [0.0, 0.0])]
    c.thin_prism[:] = [float(v) for v in cam.get("thin_prism", [0.0] * 4)]
    c.max_angle = float(cam.get("max_angle", 0.0))
    c.pose_start[:] = [float(v) for v in cam["pose_start"]]
    c.pose_end[:] = [float(v) for v in cam.get("pose_end", cam["pose_start"])]
    return c


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def higher_msb(n):
    return int(lib().oracle_higher_msb(C.c_uint32(n)))


def pose_matrices(cam: dict):
    c = make_camera(cam)
    a = np.zeros((3, 4), np.float32); b = np.zeros((3, 4), np.float32); d = np.zeros((3, 4), np.float32)
    lib().oracle_pose_matrices(C.byref(c), _p(a), _p(b), _p(d))
    return a, b, d


def forward(cam: dict, W, H, density12, sph48, ray_ori, ray_dir, sh_degree=3, params=None, threads=None):
    """Full forward. Returns dict of every intermediate buffer of SURVEY §8a plus outputs."""
    L = lib()
    prm = params or default_params()
    c = make_camera(cam)
    d12 = _f32(density12); sph = _f32(sph48)
    ro = _f32(ray_ori).reshape(-1, 3); rd = _f32(ray_dir).reshape(-1, 3)
    N = d12.shape[0]
    assert d12.shape == (N, 12) and sph.shape == (N, 48) and ro.shape[0] == W * H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    out = dict(
        tiles_count=np.zeros(N, np.uint32), proj_pos=np.zeros((N, 2), np.float32),
        conic_opacity=np.zeros((N, 4), np.float32), extent=np.zeros((N, 2), np.float32),
        depth=np.zeros(N, np.float32), feat=np.zeros((N, 3), np.float32), visibility=np.zeros(N, np.int32),
    )
    L.oracle_project(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), C.c_uint32(N), C.c_int(sh_degree),
                     _p(d12), _p(sph), _p(out["tiles_count"]), _p(out["proj_pos"]), _p(out["conic_opacity"]),
                     _p(out["extent"]), _p(out["depth"]), _p(out["feat"]), _p(out["visibility"]))
    out["tiles_offset"] = np.zeros(N, np.uint32)
    M = int(L.oracle_scan(C.c_uint32(N), _p(out["tiles_count"]), _p(out["tiles_offset"]))) if N else 0
    out["M"] = M
    keys = np.zeros(M, np.uint64); ids = np.zeros(M, np.uint32)
    if M:
        L.oracle_expand(C.byref(prm), C.c_int(W), C.c_int(H), C.c_uint32(N), _p(out["tiles_offset"]),
                        _p(out["proj_pos"]), _p(out["conic_opacity"]), _p(out["extent"]), _p(out["depth"]),
                        _p(keys), _p(ids))
    out["unsorted_keys"], out["unsorted_ids"] = keys, ids
    skeys = np.zeros(M, np.uint64); sids = np.zeros(M, np.uint32)
    end_bit = 32 + higher_msb(T)
    out["end_bit"] = end_bit
    if M:
        L.oracle_sort_pairs(C.c_uint32(M), C.c_int(end_bit), _p(keys), _p(ids), _p(skeys), _p(sids))
    out["sorted_keys"], out["sorted_ids"] = skeys, sids
    ranges = np.zeros((T, 2), np.uint32)
    if M:
        L.oracle_tile_ranges(C.c_uint32(M), C.c_uint32(T), _p(skeys), _p(ranges))
    out["tile_ranges"] = ranges
    # output initial values as allocated by the reference (splatRaster.cpp:196-199)
    rgba = np.zeros((H, W, 4), np.float32); dist = np.full((H, W, 1), 1e6, np.float32)
    hits = np.zeros((H, W, 1), np.float32)
    trav = C.c_uint64(0)
    tile_trav = np.zeros(T, np.uint32)
    if M:  # zero intersections => early return with untouched outputs (gutRenderer.cu:323-325)
        L.oracle_set_tile_traversed_out(_p(tile_trav))
        L.oracle_render(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), _p(d12), _p(out["feat"]),
                        _p(ro), _p(rd), _p(ranges), _p(sids), _p(rgba), _p(dist), _p(hits), C.byref(trav))
        L.oracle_set_tile_traversed_out(None)
    out.update(rgba=rgba, dist=dist, hits=hits, traversed_fwd=int(trav.value), tile_traversed_fwd=tile_trav,
               _inputs=(d12, sph, ro, rd, sh_degree, W, H))
    return out


def debug_ray(cam: dict, fwd: dict, px, py, params=None, max_entries=4096):
    """[n,8] float64: id, d2, response, alpha, noise estimate nu, accepted, T after, |gro| of the entries pixel (px, py) walks."""
    L = lib()
    prm = params or default_params()
    c = make_camera(cam)
    d12, sph, ro, rd, sh_degree, W, H = fwd["_inputs"]
    out = np.zeros((max_entries, 8), np.float64)
    L.oracle_debug_ray.restype = C.c_int
    n = L.oracle_debug_ray(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), _p(d12), _p(ro), _p(rd), _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]),
                           C.c_int(int(px)), C.c_int(int(py)), _p(out), C.c_int(max_entries))
    return out[:n]


def render_margins(cam: dict, fwd: dict, params=None, budget_bound=None):
    """budget_bound (e.g. 12.0): returns (margins, budget) with budget [H,W,2] float32 = the per-pixel flip budget (how far decisions
    within that many noise widths of a threshold may move the pixel's colour; by how many hits its count may differ), see gut_oracle.c.
    Per-pixel decision margins of a forward() result's compositing (oracle_render_margins): [H,W,2] float32,
    channel 0 = hit/no-hit thresholds (min_response, min_alpha), channel 1 = early termination (min_transmittance),
    both in units of the estimated fp32 noise of the compared quantity (< ~1: a different but equally valid fp32 evaluation
    of the same formula may decide differently)."""
    L = lib()
    prm = params or default_params()
    c = make_camera(cam)
    d12, sph, ro, rd, sh_degree, W, H = fwd["_inputs"]
    rgba = np.zeros((H, W, 4), np.float32); dist = np.full((H, W, 1), 1e6, np.float32); hits = np.zeros((H, W, 1), np.float32)
    margins = np.full((H, W, 2), np.finfo(np.float32).max, np.float32)
    budget = np.zeros((H, W, 2), np.float32) if budget_bound is not None else None
    if fwd["M"]:
        if budget is not None:
            L.oracle_set_pixel_budget_out(_p(budget), C.c_float(float(budget_bound)))
        L.oracle_render_margins(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), _p(d12), _p(fwd["feat"]), _p(ro), _p(rd),
                                _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]), _p(rgba), _p(dist), _p(hits), _p(margins))
        L.oracle_set_pixel_budget_out(None, C.c_float(0.0))
        assert np.array_equal(rgba, fwd["rgba"])
    return margins if budget is None else (margins, budget)


def render_kbuffer(cam: dict, fwd: dict, K=16, params=None, max_order=0, margins=False, budget_bound=None, ghosts=False):
    """Sorted-variant compositing (k_buffer_size=K) on top of a forward() result's tile lists.  Returns rgba, dist, hits and,
    if max_order > 0, the per-pixel composited particle order (order_ids [P,max_order] int32 -1 padded, order_count [P]).

    margins=True (tests only; gut_oracle.c: render_kbuffer_impl) adds
      margins [H,W,3] float32: how close the ray's decisions came to flipping, in estimated fp32 noise widths of the compared
        quantity, the unit of render_margins: channel 0 hit / no-hit (response against min_kernel_density, alpha against
        alpha_threshold, hit_t against the ray's tmin / tmax), channel 1 early termination (T against min_transmittance),
        channel 2 ORDER (the gap between a hit's distance and each pending hit it is compared with on insertion, against the
        noise of the two distances; bit-equal geometry has no margin: the insertion rule decides);
      order_nu [P,max_order] float32: the response's noise estimate of every recorded entry;
      walk [P,2] int32: list entries the ray evaluated; accepted hits still pending in its buffer when it terminated (never composited).
    budget_bound (e.g. ROW_FLIP_BOUND) adds pixel_budget [H,W,2] float32 with the semantics of render_margins(budget_bound=):
      how far the decisions within that many widths may move the pixel (2 alpha T per hit / no-hit decision, 2 T for the
      termination, 2 alpha_i alpha_j T per order comparison) and by how many hits its count may differ.
    ghosts=True (needs budget_bound and max_order) adds ghost_ids [P,max_order] / ghost_count [P]: the order of the ALTERNATIVE walk
      that takes every nearly accepted entry as a hit, decides every near order comparison the other way and walks a nearly
      terminated ray on: a composite another fp32 evaluation may arrive at on that pixel (kbuffer_backward budgets its rows)."""
    L = lib()
    prm = params or default_params()
    c = make_camera(cam)
    d12, sph, ro, rd, sh_degree, W, H = fwd["_inputs"]
    rgba = np.zeros((H, W, 4), np.float32); dist = np.full((H, W, 1), 1e6, np.float32); hits = np.zeros((H, W, 1), np.float32)
    oc = np.zeros(W * H, np.int32)
    oi = np.full((W * H, max(1, max_order)), -1, np.int32)
    out = dict(rgba=rgba, dist=dist, hits=hits, order_ids=oi, order_count=oc)
    extras = margins or budget_bound is not None or ghosts
    if extras:
        out["margins"] = np.full((H, W, 3), np.finfo(np.float32).max, np.float32)
        out["order_nu"] = np.zeros(oi.shape, np.float32)
        out["walk"] = np.zeros((W * H, 2), np.int32)
        if budget_bound is not None:
            out["pixel_budget"] = np.zeros((H, W, 2), np.float32)
        if ghosts:
            assert budget_bound is not None and max_order > 0
            out["ghost_ids"] = np.full(oi.shape, -1, np.int32)
            out["ghost_count"] = np.zeros(W * H, np.int32)
    if fwd["M"] and not extras:
        L.oracle_render_kbuffer(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), C.c_int(K), _p(d12), _p(fwd["feat"]), _p(ro), _p(rd),
                                _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]), _p(rgba), _p(dist), _p(hits),
                                _p(oi) if max_order else None, _p(oc), C.c_int(max_order))
    elif fwd["M"]:
        bound = C.c_float(float(budget_bound) if budget_bound is not None else 0.0)
        head = (C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), C.c_int(K), _p(d12), _p(fwd["feat"]), _p(ro), _p(rd),
                _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]))
        L.oracle_render_kbuffer_margins(*head, _p(rgba), _p(dist), _p(hits), _p(oi) if max_order else None, _p(oc), C.c_int(max_order),
                                        _p(out["margins"]), _p(out["pixel_budget"]) if budget_bound is not None else None, bound,
                                        _p(out["order_nu"]) if max_order else None, C.c_int(0), _p(out["walk"]))
        if ghosts:
            L.oracle_render_kbuffer_margins(*head, None, None, None, _p(out["ghost_ids"]), _p(out["ghost_count"]), C.c_int(max_order),
                                            None, None, bound, None, C.c_int(1), None)
    return out


def kbuffer_backward(cam: dict, fwd: dict, K, rgba_grad, dist_grad=None, params=None, flip_bound=None, reference_undo_colour=False,
                     max_order=None):
    """Backward of the sorted variant: float64 autograd of per_ray_torch's ordered composite on the order render_kbuffer recorded
    (the exact reference: true derivatives incl. min(max_alpha, .) and the hit distance).  Returns dict(ref = the render_kbuffer
    result with margins, dens_g [N,12] f64, sph_g [N,48] f64, feat_g [N,3] f64) and, with flip_bound, budget [N,10] f64 in the
    layout of backward(flip_bound=): columns 0..4 (positions, density, rotation, scale, colour) what another equally valid fp32
    evaluation may move the row by —
      * on a ray with ANY decision (hit / no-hit, range, termination, order) within flip_bound widths, every composited entry's row is
        budgeted with its whole |contribution| from that pixel (a swap or a flipped hit changes T and what lies behind for all);
      * where the alternative walk (render_kbuffer(ghosts=True): near hits taken, near comparisons decided the other way, a near
        termination walked on) differs from the real one, every entry of THAT composite adds its |contribution| there as well: two
        composites differ by at most the sum of their magnitudes, whatever the alphas (an entry that moves in front of an
        alpha = 0.99 neighbour gains 100 x its weight);
    columns 5..9 the fp32 conditioning: sum over hits of (relative fp32 noise of the hit) x |contribution|
    (per_ray_torch.ordered_backward)."""
    import importlib
    import torch
    prt = importlib.import_module("oracle.per_ray_torch")
    prm = params or default_params()
    d12, sph, ro, rd, sh_degree, W, H = fwd["_inputs"]
    N = d12.shape[0]
    if max_order is None:
        max_order = int(render_kbuffer(cam, fwd, K=K, params=prm)["order_count"].max(initial=0)) + 64    # room for the alternative walk's extra entries
    ref = render_kbuffer(cam, fwd, K=K, params=prm, max_order=max_order, margins=True, budget_bound=flip_bound, ghosts=flip_bound is not None)
    assert int(ref["order_count"].max(initial=0)) <= max_order
    Lmax = max(1, int(ref["order_count"].max(initial=0)))
    rg = _f32(rgba_grad).reshape(H * W, 4)
    dg = None if dist_grad is None else _f32(dist_grad).reshape(H * W)
    p64 = dict(positions=d12[:, 0:3], density=d12[:, 3:4], rotation=d12[:, 4:8], scale=d12[:, 8:11], features=sph)
    kw = dict(sh_degree=sh_degree, kernel_degree=int(prm.kernel_degree), max_alpha=float(prm.max_alpha), reference_undo_colour=reference_undo_colour)
    res = prt.ordered_backward(p64, cam["pose_start"], ro, rd, ref["order_ids"][:, :Lmax], ref["order_count"], rg, dg,
                               nu=ref["order_nu"][:, :Lmax], **kw)
    out = dict(ref=ref, dens_g=res["dens_g"], sph_g=res["sph_g"], feat_g=res["feat_g"], rgba=res["rgba"], dist=res["dist"])
    if flip_bound is None:
        return out
    budget = np.zeros((N, 10), np.float64)
    budget[:, 5:] = res["noise"]
    prone = np.nonzero(ref["margins"].reshape(H * W, 3).min(-1) < float(flip_bound))[0]
    gprone = np.nonzero((ref["ghost_ids"] != ref["order_ids"]).any(1))[0]      # the alternative walk differs from the real one
    out["prone_pixels"], out["ghost_pixels"] = prone, gprone
    if prone.size:
        ids = ref["order_ids"][prone, :Lmax]
        ok = (np.arange(Lmax)[None, :] < ref["order_count"][prone, None]).reshape(-1)
        con = res["contrib"][prone].reshape(-1, 5)[ok]
        for j in range(5):
            np.add.at(budget[:, j], ids.reshape(-1)[ok], con[:, j])
    if gprone.size:
        assert int(ref["ghost_count"].max()) <= max_order
        Lg = max(1, int(ref["ghost_count"][gprone].max()))
        gids, gcnt = ref["ghost_ids"][gprone, :Lg], ref["ghost_count"][gprone]
        g = prt.ordered_backward(p64, cam["pose_start"], ro.reshape(-1, 3)[gprone], rd.reshape(-1, 3)[gprone], gids, gcnt, rg[gprone],
                                 None if dg is None else dg[gprone], **kw)
        sel = (np.arange(Lg)[None, :] < gcnt[:, None]).reshape(-1)
        con = g["contrib"].reshape(-1, 5)[sel]
        for j in range(5):
            np.add.at(budget[:, j], gids.reshape(-1)[sel], con[:, j])
    out["budget"] = budget
    return out


def backward(cam: dict, fwd: dict, rgba_grad, dist_grad, params=None, flip_bound=None):
    """Backward for a forward() result. Returns (density_grad [N,12] f64, sph_grad [N,48] f64, feat_grad [N,3] f64).
    flip_bound (e.g. 6.0): additionally returns, as a 4th element, [N,10] f64: columns 0..4 the per-Gaussian flip budget
    (positions, density, rotation, scale, colour) — how far a different but equally valid fp32 evaluation may move each gradient
    row because a hit / no-hit decision within `flip_bound` noise widths of its threshold flips — and columns 5..9 the fp32
    conditioning of the same rows, sum over hits of eps * nu * |contribution| (gut_oracle.c: render_bwd_impl)."""
    L = lib()
    prm = params or default_params()
    c = make_camera(cam)
    d12, sph, ro, rd, sh_degree, W, H = fwd["_inputs"]
    N = d12.shape[0]
    rg = _f32(rgba_grad).reshape(H, W, 4); dg = _f32(dist_grad).reshape(H, W, 1)
    dens_g = np.zeros((N, 12), np.float64); feat_g = np.zeros((N, 3), np.float64)
    sph_g = np.zeros((N, 48), np.float64)
    trav = C.c_uint64(0)
    budget = np.zeros((N, 10), np.float64) if flip_bound is not None else None
    tile_trav = np.zeros(fwd["tile_ranges"].shape[0], np.uint32)
    if fwd["M"]:
        L.oracle_set_tile_traversed_out(_p(tile_trav))
    if fwd["M"] and budget is not None:
        L.oracle_render_bwd_budget(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), _p(d12), _p(fwd["feat"]),
                                   _p(ro), _p(rd), _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]),
                                   _p(fwd["rgba"]), _p(rg), _p(fwd["dist"]), _p(dg), _p(dens_g), _p(feat_g), C.byref(trav),
                                   _p(budget), C.c_float(float(flip_bound)))
    elif fwd["M"]:
        L.oracle_render_bwd(C.byref(prm), C.byref(c), C.c_int(W), C.c_int(H), _p(d12), _p(fwd["feat"]),
                            _p(ro), _p(rd), _p(fwd["tile_ranges"]), _p(fwd["sorted_ids"]),
                            _p(fwd["rgba"]), _p(rg), _p(fwd["dist"]), _p(dg), _p(dens_g), _p(feat_g), C.byref(trav))
    if fwd["M"]:
        L.oracle_project_bwd(C.byref(c), C.c_uint32(N), C.c_int(sh_degree), _p(d12), _p(fwd["tiles_count"]),
                             _p(fwd["feat"]), _p(feat_g), _p(sph_g))
    L.oracle_set_tile_traversed_out(None)
    fwd["traversed_bwd"] = int(trav.value)
    fwd["tile_traversed_bwd"] = tile_trav
    if budget is not None:
        return dens_g, sph_g, feat_g, budget
    return dens_g, sph_g, feat_g


# ---- the per-hit units, one call each (tests/test_cpu_reference_hits.py, tests/golden/gen_hit_golden.py) ----
REF_HITS_SO = os.path.join(_HERE, "_ref", "libgut_refhits.so")


class HitUnits:
    """The per-hit functions of ONE library behind one Python surface: `HitUnits()` the oracle's own (gut_oracle.c: oracle_kernel_response
    ... oracle_quat_to_rows, each a wrapper of the static function the passes use), `HitUnits.reference()` the reference's own header
    compiled for the host (oracle/ref_host/ref_hits.cpp -> oracle/_ref/libgut_refhits.so, built by `make -C oracle _ref` where the
    reference tree is at hand; None where it is not).  Both take and return float32 arrays in the same layout."""

    def __init__(self, handle=None, prefix="oracle_"):
        self.h = handle if handle is not None else lib()
        self.is_reference = prefix != "oracle_"
        f = lambda name: getattr(self.h, prefix + name)
        self._resp, self._resp_grad = f("kernel_response" if not self.is_reference else "particle_response"), \
            f("kernel_response_grad" if not self.is_reference else "particle_response_grd")
        self._resp.restype = C.c_float; self._resp.argtypes = [C.c_int, C.c_float]
        self._resp_grad.restype = C.c_float; self._resp_grad.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
        self._hit = f("hit_bwd_step" if not self.is_reference else "process_hit_bwd")
        self._hit.restype = C.c_int; self._hit.argtypes = [C.c_int] + [C.c_void_p] * 10
        self._sh = f("sh_radiance" if not self.is_reference else "radiance_from_sph")
        self._sh.restype = None; self._sh.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._sh_bwd = f("sh_radiance_bwd" if not self.is_reference else "radiance_from_sph_bwd")
        self._sh_bwd.restype = None; self._sh_bwd.argtypes = [C.c_int] + [C.c_void_p] * 4
        self._quat = f("quat_to_rows" if not self.is_reference else "quaternion_to_matrix")
        self._quat.restype = None; self._quat.argtypes = [C.c_void_p, C.c_void_p]

    @classmethod
    def reference(cls):
        return cls(C.CDLL(REF_HITS_SO), "ref_") if os.path.exists(REF_HITS_SO) else None

    def response(self, degree, d2):
        return np.float32(self._resp(int(degree), float(np.float32(d2))))

    def response_grad(self, degree, d2, resp, resp_grad):
        return np.float32(self._resp_grad(int(degree), float(np.float32(d2)), float(np.float32(resp)), float(np.float32(resp_grad))))

    def hit_bwd(self, degree, ray_ori, ray_dir, particle12, feat3, thresholds, finals, cot, state):
        """One processHitBwd step.  thresholds = (min response, min alpha, min transmittance); finals / state = (transmittance,
        radiance[3], depth); cot = (transmittance gradient, radiance gradient[3], depth gradient).  Returns (accepted, state after
        [5], density gradient [11], feature gradient [3])."""
        a = [_f32(v).reshape(-1) for v in (ray_ori, ray_dir, particle12, feat3, thresholds, finals, cot)]
        st = _f32(state).reshape(-1).copy()
        g11 = np.zeros(11, np.float32); g3 = np.zeros(3, np.float32)
        assert [v.size for v in a] == [3, 3, 12, 3, 3, 5, 5] and st.size == 5
        acc = self._hit(int(degree), *[_p(v) for v in a], _p(st), _p(g11), _p(g3))
        return int(acc), st, g11, g3

    def sh_radiance(self, deg, sph48, dir3, clamped):
        s, d = _f32(sph48).reshape(-1), _f32(dir3).reshape(-1)
        assert s.size == 48 and d.size == 3
        out = np.zeros(3, np.float32)
        self._sh(int(deg), _p(s), _p(d), int(bool(clamped)), _p(out))
        return out

    def sh_radiance_bwd(self, deg, dir3, rad_grad3, radiance_unclamped3):
        """[48] coefficient gradient.  The reference's is float32; the oracle's takes a float64 cotangent and returns float64."""
        d, u = _f32(dir3).reshape(-1), _f32(radiance_unclamped3).reshape(-1)
        if self.is_reference:
            g = _f32(rad_grad3).reshape(-1); out = np.zeros(48, np.float32)
        else:
            g = np.ascontiguousarray(np.asarray(rad_grad3, np.float64)).reshape(-1); out = np.zeros(48, np.float64)
        assert d.size == 3 and u.size == 3 and g.size == 3
        self._sh_bwd(int(deg), _p(d), _p(g), _p(u), _p(out))
        return out

    def quat_rows(self, q_wxyz):
        q = _f32(q_wxyz).reshape(-1); out = np.zeros(9, np.float32)
        assert q.size == 4
        self._quat(_p(q), _p(out))
        return out.reshape(3, 3)


def world_rays(cam: dict, ray_ori, ray_dir):
    """The world-space rays the compositing passes walk (make_ray: sensor -> world, the scene-box test): origins [P,3], directions
    [P,3] float32, alive [P] int32."""
    c = make_camera(cam)
    ro = _f32(ray_ori).reshape(-1, 3); rd = _f32(ray_dir).reshape(-1, 3)
    o = np.zeros_like(ro); d = np.zeros_like(rd); alive = np.zeros(ro.shape[0], np.int32)
    lib().oracle_world_rays(C.byref(c), C.c_uint32(ro.shape[0]), _p(ro), _p(rd), _p(o), _p(d), _p(alive))
    return o, d, alive


def view_direction(cam: dict, position3):
    """normalize(position - sensor position) as oracle_project / oracle_project_bwd evaluate it: the direction of a Gaussian's SH."""
    c = make_camera(cam)
    p = _f32(position3).reshape(-1); out = np.zeros(3, np.float32)
    lib().oracle_view_direction(C.byref(c), _p(p), _p(out))
    return out
