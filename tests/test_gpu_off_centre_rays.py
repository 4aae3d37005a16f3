"""Rays that do not start at the sensor position, on the device (tests/off_centre_cases.py: the origin planes and which tiles they
move to the un-centred instantiations; tests/test_cpu_off_centre_cases.py: the preconditions on the oracle and float64 alone).

The compositing kernels and the walk are instantiated twice on the block-uniform `centred` (gut_render_common.h: make_ray).  The
un-centred forms have arithmetic of their own — the M e product added to the canonical origin (K6, k_walk, the sorted eval_entry),
no strip culling, e carried through both rank-1 factorisations of K7, the `ori1 < 3e38` clause of K7's usable test — and every
camera helper of the package returns centred rays, so nothing else in the suite runs them.  Here they meet the oracle with the
helpers and the constants the centred tests use (tests/test_gpu_parity.py, tests/common.py): nothing is tuned for them.

  compositors   cases x {shift, sweep, half}: integer buffers and projection floats bit-identical to the oracle AND to the device's
                own centred run (K1 reads no rays); image per pixel against margins and budget; traversal depths; gradient blocks;
                every row with and without a distance gradient (K7's two forms); lazy order on / off
  exact         half: tiles left of the cut keep the bits of the all-centred render; -0.0f origins are the +0 run bit for bit
  variants      sorted forward / backward at K = 4, 16; generalised kernels; sorted x generalised; the raw / model-field entry
                points; a rolling shutter; NaN / inf origins
  walks         the five sinks of k_walk on three cases x {shift, sweep} with the assertions of their one-view tests; decision
                equality with the forward at 1e8 (pixel, entry) evaluations; back-projection; mesh.view_of
  pose          gut_set_pose_gradient against its definition on the rows of the same backward"""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import off_centre_cases as oc
from tests import surface_reference as sr
from tests import test_gpu_attribute_gradient as t_attribute_gradient
from tests import test_gpu_attributes as t_attributes
from tests import test_gpu_contribution as t_contribution
from tests import test_gpu_parity as P
from tests import test_gpu_pose_gradient as t_pose
from tests import test_gpu_raw_path as t_raw
from tests import test_gpu_surface as t_surface
from tests import test_gpu_weighted_contribution as t_weighted
from tests.common import (COLOUR_TOL, GRAD_BLOCKS, ROW_FLIP_BOUND, cams, check_colour_outliers, densified_like_scene, make_view, pose,
                          rel_l2, scenes, to_batch)

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
mesh = importlib.import_module("3dgrut_amd.mesh")
surface = importlib.import_module("3dgrut_amd.surface")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"

CASES = ("c1_pinhole_128", "ragged_100x70", "fisheye_distorted", "dense_big_splats")
PLANES = ("shift", "sweep", "half")
INT_KEYS = ("tiles_count", "tiles_offset", "unsorted_ids", "sorted_ids")
KEY_KEYS = ("unsorted_keys", "sorted_keys")
FLOAT_KEYS = ("proj_pos", "conic_opacity", "extent", "depth", "feat")


@functools.lru_cache(maxsize=None)
def _scene_view(name):
    mk, kind, W, H, (eye, tgt), kw = P.CASES[name]
    return mk(), make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)


def _buffers(raster):
    out = {k: raster.debug_buffer(k).cpu().numpy().view(np.uint32).copy() for k in INT_KEYS + FLOAT_KEYS}
    out.update({k: raster.debug_buffer(k).cpu().numpy().view(np.uint64).copy() for k in KEY_KEYS})
    out["tile_ranges"] = raster.debug_buffer("tile_ranges").cpu().numpy().view(np.uint32).reshape(-1, 2).copy()
    return out


def _image(out):
    return dict(rgba=np.concatenate([out["pred_rgb"][0].detach().cpu().numpy(), out["pred_opacity"][0].detach().cpu().numpy()], -1),
                dist=out["pred_dist"][0].detach().cpu().numpy(), hits=out["hits_count"][0].detach().cpu().numpy())


def _grads(H, W, seed=11):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(H, W, 4)).astype(np.float32), (0.1 * rng.normal(size=(H, W, 1))).astype(np.float32)


def _check_against_the_oracle(label, sc, view, model, d12, sph, ref, rgba_grad, dist_grad, conf=None, params=None):
    """One forward and backward of Tracer.render on `view` against the oracle result `ref`: the statements of
    test_forward_buffers_and_image and test_backward_gradients.  Returns (result of _run_gpu, its buffers, its image)."""
    W, H = view["W"], view["H"]
    res = P._run_gpu(sc, view, 3, rgba_grad=rgba_grad, dist_grad=dist_grad, model=model, render_conf=conf)
    raster = res["tracer"].tracer_wrapper
    st = raster.stats()
    assert st["num_intersections"] == ref["M"] and st["num_visible"] == int((ref["tiles_count"] > 0).sum())
    buf = _buffers(raster)
    for key in INT_KEYS + KEY_KEYS:
        assert np.array_equal(buf[key], ref[key]), (label, key)
    assert np.array_equal(buf["tile_ranges"], ref["tile_ranges"]), label
    P._check_ordered_ids(raster, ref)
    for key in FLOAT_KEYS:
        exp = np.ascontiguousarray(ref[key]).reshape(-1).view(np.uint32)
        assert np.array_equal(buf[key], exp), f"{label}/{key}: {(buf[key] != exp).sum()} of {exp.size} words differ"
    img = _image(res["out"])
    margins, pixel_budget = oracle.render_margins(view["oracle_cam"], ref, params=params, budget_bound=ROW_FLIP_BOUND)
    rep = check_colour_outliers(img["rgba"], img["hits"], ref, margins, label=label, dist_gpu=img["dist"], budget=pixel_budget)
    assert rep["outliers"] <= 1e-3 * rep["pixels"]
    assert st["traversed_fwd"] == ref["traversed_fwd"], label
    dens_g, sph_g, _ = oracle.backward(view["oracle_cam"], ref, rgba_grad, dist_grad if dist_grad is not None else np.zeros((H, W, 1), np.float32),
                                       params=params)
    for k, e in P._activated_grads(model, dens_g, sph_g).items():
        g = getattr(model, k).grad.cpu().numpy()
        assert np.isfinite(g).all(), (label, k)
        err = rel_l2(g, e)
        print(f"[blocks {label}] {k}: rel L2 {err:.3e}")
        assert err <= 2e-3, f"{label}/{k}: rel L2 {err}"
    assert raster.stats()["traversed_bwd"] == ref["traversed_bwd"], label
    return res, buf, img


# ---- the compositors, default path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("name", CASES)
def test_compositors_against_the_oracle(name, plane):
    sc, view0 = _scene_view(name)
    view = oc.off_centre(view0, plane)
    W, H = view["W"], view["H"]
    un = oc.uncentred_tiles(view)
    if plane == "shift":
        assert un.all()
    elif plane == "sweep":
        assert (~un).sum() <= 1
    else:
        assert not un[:, :2].any() and un[:, 2:].all()
    model, d12, sph = P._oracle_inputs(sc, 3)
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    rgba_grad, dist_grad = _grads(H, W)
    # the device's own centred run: K1 reads no rays, every buffer it writes must not depend on the origin plane
    centred = P._run_gpu(sc, view0, 3, model=model)
    buf0, img0 = _buffers(centred["tracer"].tracer_wrapper), _image(centred["out"])
    label = f"off-centre {name}/{plane}"
    res, buf, img = _check_against_the_oracle(label, sc, view, model, d12, sph, ref, rgba_grad, dist_grad)
    for key in buf0:
        assert np.array_equal(buf[key], buf0[key]), f"{label}: {key} differs from the centred run's"
    moved = float(np.abs(img["rgba"] - img0["rgba"]).max())
    print(f"[{label}] {int(un.sum())} of {un.size} tiles un-centred; the image moves by {moved:.3f} against the centred render")
    assert moved > 100 * COLOUR_TOL
    # every row, with and without the distance gradient: K7's two forms
    for dg in (None, dist_grad):
        P.check_rows_in_activated_space(f"{label}/dist={int(dg is not None)}", view, d12, sph, 3, ref, rgba_grad, dg)


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("name", CASES)
def test_lazy_tile_order_is_equivalent_off_centre(name, plane):
    """test_lazy_tile_order_is_equivalent's statements on the un-centred forms of K6 (lazy and eager) and K7."""
    sc, view0 = _scene_view(name)
    view = oc.off_centre(view0, plane)
    W, H = view["W"], view["H"]
    rgba_grad = np.random.default_rng(3).normal(size=(H, W, 4)).astype(np.float32)
    model, d12, sph = P._oracle_inputs(sc, 3)
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    a = P._run_gpu(sc, view, 3, rgba_grad=rgba_grad, model=model, lazy=False)
    ga = {k: getattr(model, k).grad.clone() for k in ("positions", "rotation", "scale", "density", "features_albedo")}
    model.zero_grad(set_to_none=True)
    b = P._run_gpu(sc, view, 3, rgba_grad=rgba_grad, model=model, lazy=True)
    assert torch.equal(a["out"]["pred_rgb"], b["out"]["pred_rgb"]) and torch.equal(a["out"]["pred_dist"], b["out"]["pred_dist"])
    assert torch.equal(a["out"]["pred_opacity"], b["out"]["pred_opacity"]) and torch.equal(a["out"]["hits_count"], b["out"]["hits_count"])
    ra, rb = a["tracer"].tracer_wrapper, b["tracer"].tracer_wrapper
    assert torch.equal(ra.debug_buffer("tile_traversed_fwd"), rb.debug_buffer("tile_traversed_fwd"))
    assert np.array_equal(rb.debug_buffer("sorted_ids").cpu().numpy().view(np.uint32), ref["sorted_ids"])
    P._check_ordered_ids(rb, ref)
    for k, g in ga.items():
        assert rel_l2(getattr(model, k).grad.cpu().numpy(), g.cpu().numpy()) <= 1e-5, k


# ---- exact properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_centred_tiles_of_the_half_plane_keep_the_centred_bits(name):
    """The `half` plane is zero for px < 40: the tiles of the columns 0..31 are wholly centred and take the centred instantiation, so
    every output bit of their pixels is the all-centred render's.  The tile column 32..47 is mixed (un-centred form, zero e on its
    left half) and may differ in the last bits; right of the cut the image moves."""
    sc, view0 = _scene_view(name)
    view = oc.off_centre(view0, "half")
    un = oc.uncentred_tiles(view)
    assert not un[:, :2].any() and un[:, 2:].all()
    model = P.gut_model(sc, 3)
    a, b = _image(P._run_gpu(sc, view0, 3, model=model)["out"]), _image(P._run_gpu(sc, view, 3, model=model)["out"])
    left = slice(0, 32)
    for key in ("rgba", "dist", "hits"):
        x, y = np.ascontiguousarray(a[key][:, left]).view(np.uint32), np.ascontiguousarray(b[key][:, left]).view(np.uint32)
        assert np.array_equal(x, y), f"{name}: {key} of {(x != y).sum()} words left of the cut differ from the centred render"
    assert float(np.abs(a["rgba"][:, oc.HALF_CUT:] - b["rgba"][:, oc.HALF_CUT:]).max()) > 100 * COLOUR_TOL


def _trace_rows(v, d12, sph, rgba_grad, dist_grad):
    """One SplatRaster.trace / trace_bwd of the activated rows on a fresh handle: outputs, rows, traversal depths, walked lists."""
    raster = gut.Tracer({"render": {}}).tracer_wrapper
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(v, DEV))
    cam = (torch.as_tensor(v["ro"], device=DEV).contiguous(), torch.as_tensor(v["rd"], device=DEV).contiguous(), None, sensor,
           poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
    d12_t, sph_t = torch.as_tensor(d12, device=DEV), torch.as_tensor(sph, device=DEV)
    rgba, dist, hits, _ = raster.trace(0, 3, d12_t, sph_t, *cam)
    g12, g48 = raster.trace_bwd(0, 3, d12_t, sph_t, *cam, rgba, torch.as_tensor(rgba_grad, device=DEV), dist, torch.as_tensor(dist_grad, device=DEV))
    return dict(rgba=rgba.cpu().numpy(), dist=dist.cpu().numpy(), hits=hits.cpu().numpy(), g12=g12.cpu().numpy().astype(np.float64),
                g48=g48.cpu().numpy().astype(np.float64), trav=raster.debug_buffer("tile_traversed_fwd").cpu().numpy(),
                ordered=raster.debug_buffer("ordered_ids").cpu().numpy())


@pytest.mark.parametrize("name", CASES)
def test_negative_zero_origins_are_centred(name):
    """-0.0f == 0.0f: a plane of negative zeros takes the centred form.  Forward outputs, traversal depths and walked lists are the
    +0 run's bit for bit.  The backward sums with float atomics, so runs of the same input differ, and by how much varies from pair
    to pair: over 28 pairs of +0 runs the largest row difference of a block spreads over a factor of 10, its relative L2 over a
    factor of 6 (measured on the MI355X; the -0 runs spread the same).  The band is therefore measured here from four +0 runs, per
    block, as the LARGEST of their six pairwise differences, and the -0 run must lie within twice that band of its NEAREST +0 run —
    in the largest row difference and in the block's relative L2 — and within the 1e-5 relative L2 the suite allows the atomic
    order everywhere.  A band of exactly 0 asks for equal bits."""
    sc, view0 = _scene_view(name)
    view = oc.off_centre(view0, "negative_zero")
    assert np.signbit(view["ro"]).all() and not oc.uncentred_tiles(view).any()
    W, H = view["W"], view["H"]
    rgba_grad, dist_grad = _grads(H, W, 7)
    model, d12, sph = P._oracle_inputs(sc, 3)
    plus = [_trace_rows(view0, d12, sph, rgba_grad, dist_grad) for _ in range(4)]
    n = _trace_rows(view, d12, sph, rgba_grad, dist_grad)
    for key in ("rgba", "dist", "hits", "trav", "ordered"):
        for p in plus:
            assert np.array_equal(p[key].view(np.uint32), n[key].view(np.uint32)), f"{name}: {key} of the -0 run differs from a +0 run"
    blocks = [(block, "g12", sl) for block, sl in GRAD_BLOCKS] + [("sh", "g48", slice(None))]
    for block, key, sl in blocks:
        row = lambda x, y: float(np.linalg.norm(x[key][:, sl] - y[key][:, sl], axis=1).max())
        l2 = lambda x, y: rel_l2(x[key][:, sl], y[key][:, sl])
        pairs = [(x, y) for i, x in enumerate(plus) for y in plus[i + 1:]]
        band_row, band_l2 = max(row(x, y) for x, y in pairs), max(l2(x, y) for x, y in pairs)
        got_row, got_l2 = min(row(n, p) for p in plus), min(l2(n, p) for p in plus)
        print(f"[negative zero {name}/{block}] run-to-run band: rows {band_row:.3e}, relative L2 {band_l2:.3e}; -0 run against its nearest "
              f"+0 run: rows {got_row:.3e}, relative L2 {got_l2:.3e}")
        assert got_row <= 2.0 * band_row and got_l2 <= 2.0 * band_l2, (name, block, got_row, band_row, got_l2, band_l2)
        assert max(l2(n, p) for p in plus) <= 1e-5


# ---- sorted and generalised kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("name", ["c1_pinhole_128", "dense_big_splats"])
def test_sorted_variant_off_centre(name, K):
    """The sorted forward and backward (eval_entry's un-centred branch) on the `shift` plane: every pixel and every row against the
    k-buffer oracle, with a distance gradient."""
    sc, view0 = _scene_view(name)
    view = oc.off_centre(view0, "shift")
    W, H = view["W"], view["H"]
    rgba_grad, dist_grad = _grads(H, W, 5)
    _, d12, sph = P._oracle_inputs(sc, 3)
    P._check_sorted_rows(f"off-centre sorted {name}/shift/K={K}", view, d12, sph, W, H, K, rgba_grad, dist_grad)


@pytest.mark.parametrize("degree", [1, 4])
def test_generalised_kernels_off_centre(degree):
    """particle_kernel_degree 1 and 4 (the kGeneral instantiations of K6 and K7) on c1_pinhole_128 with the `sweep` plane."""
    sc, view0 = _scene_view("c1_pinhole_128")
    view = oc.off_centre(view0, "sweep")
    W, H = view["W"], view["H"]
    prm = oracle.default_params()
    prm.kernel_degree = degree
    conf = {"particle_kernel_degree": degree}
    model, d12, sph = P._oracle_inputs(sc, 3)
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3, params=prm)
    rgba_grad, dist_grad = _grads(H, W, 17)
    label = f"off-centre degree {degree}/sweep"
    _check_against_the_oracle(label, sc, view, model, d12, sph, ref, rgba_grad, dist_grad, conf=conf, params=prm)
    for dg in (None, dist_grad):
        P.check_rows_in_activated_space(f"{label}/dist={int(dg is not None)}", view, d12, sph, 3, ref, rgba_grad, dg, conf=conf, params=prm)


def test_sorted_generalised_kernel_off_centre():
    sc, view0 = _scene_view("c1_pinhole_128")
    view = oc.off_centre(view0, "shift")
    W, H = view["W"], view["H"]
    rgba_grad, dist_grad = _grads(H, W, 15)
    _, d12, sph = P._oracle_inputs(sc, 3)
    P._check_sorted_rows("off-centre sorted K=8/degree 4/shift", view, d12, sph, W, H, 8, rgba_grad, dist_grad, kernel_degree=4)


# ---- raw / model-field entry points, rolling shutter ----------------------------------------------------------------------------
def test_raw_and_model_field_entry_points_off_centre():
    """gut_trace_raw_model_fields / gut_trace_bwd_model_fields (Tracer.raw_parameters) on ragged_100x70 with the `sweep` plane: the
    checks of tests/test_gpu_raw_path.py — packed rows, integer buffers, image, every row of the six raw-parameter gradients."""
    sc, view0 = _scene_view("ragged_100x70")
    view = oc.off_centre(view0, "sweep")
    t_raw._check_raw_path("off-centre ragged_100x70/sweep", P.gut_model(sc, 3), view, 3, t_raw._grad_image(view["H"], view["W"], 31))


def test_rolling_shutter_off_centre():
    """Distinct start and end poses with the `shift` plane (the un-centred and the rolling instantiations compose): the case of
    test_raw_path_with_a_rolling_shutter, shutter type 1, forward and backward."""
    shutter = 1
    sc = scenes.scene_c1(700, 40 + shutter)
    W, H = 96, 80
    view0 = make_view("pinhole", W, H, cams.look_at_c2w((0.1, 0.0, -3.0), (0, 0, 0)), fx=90)
    view = oc.off_centre(view0, "shift")
    tq_end = pose.sensor_pose_from_c2w(cams.look_at_c2w((0.25, -0.1, -2.9), (0.05, 0.0, 0.0))).T_world_sensors[0]
    ocam = dict(view["oracle_cam"], shutter=shutter, pose_end=tq_end)
    d12, sph = scenes.pack_density(sc), sc["features"]
    moved = oracle.forward(ocam, W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)["rgba"]
    still = oracle.forward(dict(view0["oracle_cam"], shutter=shutter, pose_end=tq_end), W, H, d12, sph, view0["ro"], view0["rd"], sh_degree=3)["rgba"]
    assert float(np.abs(moved - still).max()) > 100 * COLOUR_TOL

    def edit(sensor):
        sensor.cam.shutter = shutter

    t_raw._check_raw_path("off-centre rolling shutter/shift", P.gut_model(sc, 3), view, 3, t_raw._grad_image(H, W, shutter), ocam=ocam,
                          sensor_edit=edit, tq_end=tq_end)


# ---- unusable origins -------------------------------------------------------------------------------------------------------------
def _unusable_view():
    sc, view0 = _scene_view("c1_pinhole_128")
    view = oc.off_centre(view0, "shift")
    H, W = view["H"], view["W"]
    ro = view["ro"].copy()
    r3 = ro.reshape(H, W, 3)
    with np.errstate(over="ignore"):
        huge = np.float64(1e39).astype(np.float32)       # beyond float32: +inf
    assert np.isposinf(huge)
    r3[40, 50] = np.nan
    r3[41, 51] = (np.inf, 0.05, 0.02)
    r3[42, 52] = huge
    r3[70, 60, 1] = np.nan                               # one component only
    r3[10:12, 100:104] = np.nan                          # a 2 x 4 block inside one wave
    r3[90:92, 20:24] = np.inf
    bad = ~np.isfinite(r3).all(-1)
    return sc, dict(view, ro=ro), bad


def _check_distances_of_the_usable_pixels(label, got, ref, bad, margins, pixel_budget):
    """The initial hit distance of an invalid ray is 1e6, and check_colour_outliers measures distances relative to the frame's largest:
    once more with the unusable pixels' distance set to 0 on both sides, so that the usable pixels are held to their own scale."""
    H, W = bad.shape
    ref0 = dict(ref, dist=np.where(bad[..., None], 0.0, ref["dist"].reshape(H, W, 1)).astype(np.float32))
    dist0 = np.where(bad[..., None], 0.0, got["dist"].reshape(H, W, 1)).astype(np.float32)
    assert float(ref0["dist"].max()) < 100.0
    check_colour_outliers(got["rgba"], got["hits"], ref0, margins, label=f"{label}/usable distances", dist_gpu=dist0, budget=pixel_budget)


def test_unusable_origins_do_not_poison_gradients():
    """test_unusable_rays_do_not_poison_gradients for the ORIGIN: NaN, +inf and 1e39 (+inf in float32) at single pixels and in
    2 x 4 blocks of the `shift` plane.  Such a ray fails the scene-box test in the reference (rayPayload.cuh:93-101: every slab
    comparison with NaN is false, tMinMax.y > tMinMax.x is false), so it is invalid, composites nothing and keeps the initial
    output values — in the oracle and on the device.  K7 evaluates its lanes with zero weights once a neighbour hits, so their
    e must be neutralised (the `ori1 < 3e38` clause of `usable`): the gradients stay finite and equal the oracle's."""
    sc, view, bad = _unusable_view()
    W, H = view["W"], view["H"]
    assert int(bad.sum()) == 4 + 8 + 8
    rgba_grad, dist_grad = _grads(H, W, 2)
    model, d12, sph = P._oracle_inputs(sc, 3)
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    assert not ref["rgba"][bad].any() and not ref["hits"][bad].any() and np.isfinite(ref["rgba"]).all()
    dens_g, sph_g, _ = oracle.backward(view["oracle_cam"], ref, rgba_grad, dist_grad)
    assert np.isfinite(dens_g).all() and np.isfinite(sph_g).all()
    label = "unusable origins"
    res, _, img = _check_against_the_oracle(label, sc, view, model, d12, sph, ref, rgba_grad, dist_grad)
    for key in ("rgba", "dist", "hits"):    # the unusable pixels themselves: the oracle's (initial) values, exactly
        assert np.array_equal(img[key][bad], ref[key][bad]), key
    _check_distances_of_the_usable_pixels(label, img, ref, bad, *oracle.render_margins(view["oracle_cam"], ref, budget_bound=ROW_FLIP_BOUND))
    for dg in (None, dist_grad):
        P.check_rows_in_activated_space(f"{label}/dist={int(dg is not None)}", view, d12, sph, 3, ref, rgba_grad, dg)


@pytest.mark.parametrize("K", [4, 16])
def test_unusable_origins_in_the_sorted_variant(K):
    sc, view, bad = _unusable_view()
    W, H = view["W"], view["H"]
    rgba_grad, dist_grad = _grads(H, W, 2)
    _, d12, sph = P._oracle_inputs(sc, 3)
    from tests import sorted_cases
    from tests.test_gpu_sorted_variant import run_sorted
    label = f"unusable origins sorted K={K}"
    P._check_sorted_rows(label, view, d12, sph, W, H, K, rgba_grad, dist_grad)
    case = sorted_cases.from_rows(label, d12, sph, view, W, H)
    got = run_sorted(case, K, rgba_grad, dist_grad)
    kb = sorted_cases.kbuffer(case, K, ROW_FLIP_BOUND)
    assert np.isfinite(got["g12"]).all() and np.isfinite(got["g48"]).all() and np.isfinite(got["rgba"]).all()
    for key in ("rgba", "dist", "hits"):
        assert np.array_equal(got[key].reshape(H, W, -1)[bad], kb[key].reshape(H, W, -1)[bad]), key
    _check_distances_of_the_usable_pixels(label, got, kb, bad, kb["margins"], kb["pixel_budget"])


# ---- the walks ------------------------------------------------------------------------------------------------------------------
WALK_CASES = [f"{base}@{plane}" for base in ("pinhole_64x48", "ragged_70x45", "fisheye") for plane in ("shift", "sweep")]
EXACT = lambda name, bases: cr.base_name(name) in bases     # the exact-identity tests keep the cases they are written for


@pytest.mark.parametrize("name", WALK_CASES)
def test_contribution_walk_off_centre(name):
    assert np.abs(cr.case(name)["view"]["ro"]).max() > 0
    t_contribution.test_scores_of_one_view(name)


@pytest.mark.parametrize("name", WALK_CASES)
def test_weighted_contribution_walk_off_centre(name):
    t_weighted.test_weighted_scores_of_one_view(name)
    if EXACT(name, ("ragged_70x45",)):
        t_weighted.test_exact_identities(name)


@pytest.mark.parametrize("name", WALK_CASES)
def test_attribute_walk_off_centre(name):
    t_attributes.test_planes_against_the_oracle(name)
    t_attributes.test_planes_against_the_devices_own_forward(name)
    t_attributes.test_adjoint_of_the_weighted_contribution_walk(name)
    if EXACT(name, ("ragged_70x45", "fisheye")):
        t_attributes.test_exact_properties(name)


@pytest.mark.parametrize("name", WALK_CASES)
def test_attribute_gradient_walk_off_centre(name):
    t_attribute_gradient.test_rows_against_the_reference(name)
    t_attribute_gradient.test_against_the_clamped_walk(name)
    t_attribute_gradient.test_adjoint_of_the_attribute_walk(name)
    if EXACT(name, ("ragged_70x45", "fisheye")):
        t_attribute_gradient.test_exact_identities(name)


@pytest.mark.parametrize("name", WALK_CASES)
def test_surface_walk_off_centre(name):
    t_surface.test_planes_against_the_reference(name)
    t_surface.test_level_mode_against_the_forwards_alpha(name)
    t_surface.test_largest_weight_mode_against_the_contribution_records(name)
    if EXACT(name, ("ragged_70x45", "fisheye")):
        t_surface.test_exact_properties(name)


def test_backprojected_surface_of_the_shift_plane_lies_on_the_oracles_hit_points():
    """surface.backproject uses rays_ori.  (a) On the reference distances of ragged_70x45@shift it gives the float64 points origin +
    distance x direction to test_backproject_on_the_device's 1e-5 of the largest coordinate.  (b) The device's own level-0.5
    distances, back-projected, lie on the oracle's hit points: where the pixel is not near, the distance is within COLOUR_TOL x
    max(1, largest distance) (test_planes_against_the_reference), so the point is within that length plus the 1e-5 of (a).
    mesh.view_of hands the origin plane of this batch to the fusion, and None for the centred one."""
    name = "ragged_70x45@shift"
    case, raster, v, d12, sph = t_surface._case_on_device(name)
    s = sr.surface_case(name)
    ref = sr.level_planes(name, 0.5)
    want = sr.backproject(s["view"], ref["distance"])
    centred_want = sr.backproject(cr.case("ragged_70x45")["view"], ref["distance"])
    batch = to_batch(s["view"], DEV)
    some = ref["distance"] > 0
    size = float(np.abs(want[some]).max())
    assert float(np.abs(want[some] - centred_want[some]).max()) > 1e-2          # the origin plane matters: |shift| = 0.06
    got = surface.backproject(batch, torch.as_tensor(ref["distance"], device=DEV)).cpu().numpy()
    assert bool(np.isnan(got[~some]).all())
    worst = float(np.abs(got[some] - want[some]).max() / size)
    t_surface._forward(raster, d12, sph, v)
    dist, ids, wgt = t_surface._surface(raster, d12, v, "level", 0.5)
    pts = surface.backproject(batch, dist).cpu().numpy()
    calm = some & ~ref["near"] & (ids.cpu().numpy() >= 0)
    far = max(1.0, float(ref["distance"].max()))
    worst_dev = float(np.abs(pts[calm] - want[calm]).max())
    print(f"[backproject off-centre] reference distances: worst {worst:.3e} of the largest coordinate; device distances: worst {worst_dev:.3e} "
          f"(bound {COLOUR_TOL * far + 1e-5 * size:.3e}) on {int(calm.sum())} pixels")
    assert worst <= 1e-5
    assert worst_dev <= COLOUR_TOL * far + 1e-5 * size
    render = dict(distance=dist, rgba=torch.zeros((case["H"], case["W"], 4), device=DEV))
    origin = mesh.view_of(batch, render)["ray_origin"]
    assert origin is not None and torch.equal(origin, batch.rays_ori.reshape(case["H"], case["W"], 3))
    assert mesh.view_of(to_batch(cr.case("ragged_70x45")["view"], DEV), render)["ray_origin"] is None


# ---- walk decisions at scale ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [None, "shift", "sweep"])
def test_walk_decisions_equal_the_forwards_at_scale(plane):
    """k_walk must make the very decisions K6 made, entry by entry: sum(pixels) == sum(hit counts), exactly, and the sum of
    weight_sum equals the sum of alpha within COLOUR_TOL x pixels with a hit — the device against its own forward, no CPU reference.
    A contraction difference of one ulp between the two kernels flips about one decision in 1e7 evaluations, which
    the 64 x 48 cases cannot see: densified_like_scene(20000, 5) at 320 x 320 makes 1.7e7 (pixel, entry) evaluations, so the scene
    is its 200000-row form at 720 x 720: 1.16e8 = 256 x the sum of the tiles' traversal depths, asserted >= 1e8."""
    sc = densified_like_scene(200000, 5)
    W = H = 720
    view = make_view("pinhole", W, H, cams.orbit_c2w(3.6, -40, 25), fx=945.0)
    if plane is not None:
        view = oc.off_centre(view, plane)
    raster = t_contribution._raster()
    v = t_contribution._device_view(view)
    d12 = torch.as_tensor(np.ascontiguousarray(scenes.pack_density(sc)), device=DEV)
    sph = torch.as_tensor(np.ascontiguousarray(sc["features"].astype(np.float32)), device=DEV)
    n = d12.shape[0]
    rgba, dist, hits, vis = t_contribution._forward(raster, d12, sph, v)
    scores = t_contribution._score(raster, d12, v, t_contribution._zeroed(n))
    torch.cuda.synchronize()
    ws, mw, px = t_contribution._host(scores)
    evaluations = 256 * int(raster.debug_buffer("tile_traversed_fwd").view(torch.int32).to(torch.int64).sum())
    hit_sum, alpha_sum, with_hit = int(hits.double().sum()), float(rgba[..., 3].double().sum()), int((hits > 0).sum())
    print(f"[walk decisions {plane}] {evaluations:.3e} (pixel, entry) evaluations; pixels {int(px.sum())} vs hit counts {hit_sum}; "
          f"sum of weight_sum {ws.sum():.6f} vs sum alpha {alpha_sum:.6f}: {abs(ws.sum() - alpha_sum) / (COLOUR_TOL * with_hit):.3e} of the bound")
    assert evaluations >= 1e8
    assert int(px.sum()) == hit_sum, f"{plane}: the walk decides differently from the forward compositor on {int(px.sum()) - hit_sum} entries"
    assert abs(ws.sum() - alpha_sum) <= COLOUR_TOL * with_hit


# ---- pose gradient --------------------------------------------------------------------------------------------------------------
def test_pose_gradient_kernel_off_centre():
    """test_kernel_equals_the_definition_on_the_rows_of_the_same_backward on pinhole_128 with the `shift` plane."""
    sc = scenes.scene_c1(1000, 0)
    act, sph = t_pose._rows(sc)
    view = oc.off_centre(make_view("pinhole", 128, 128, cams.look_at_c2w(*t_pose.LOOK_AT)), "shift")
    raster = gut.SplatRaster({"render": {}})
    cam_pos = np.asarray(view["c2w"], np.float64)[:3, 3]
    for seed in range(8):
        out8, dens_g, tiles = t_pose._backward_with_pose_gradient(raster, view, act, sph, seed)
        terms = pose.pose_gradient_terms(act, dens_g, cam_pos)
        ref, S = terms.sum(0).cpu(), terms.abs().sum(0).cpu()
        if bool((ref.abs() >= 1e-3 * S).all()):
            break
    else:
        pytest.fail("no cotangent seed below 8 gives |ref_k| >= 1e-3 S_k for every k")
    err = (out8[:6] - ref).abs()
    print(f"[pose kernel off-centre] seed {seed} |ref|/S {(ref.abs() / S).tolist()} err/S {(err / S).tolist()} rows {int(out8[6])}")
    assert bool((S > 0).all())
    assert bool((err <= 1e-5 * S).all()), (err / S).tolist()
    assert float(out8[6]) == float((tiles != 0).sum()) > 0 and float(out8[7]) == 0.0
