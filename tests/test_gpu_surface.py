"""gut_trace_surface on the device: the distance, id and weight planes of both modes against the CPU reference
(tests/surface_reference.py, asserted by tests/test_cpu_surface.py) wherever no decision of the pixel is near its threshold; the
properties that hold exactly, against the device's own forward and contribution records; that it disturbs nothing; its refusals;
empty inputs; the points of the wall; the trainer's command line."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import surface_reference as sr
from tests.common import COLOUR_TOL, cams, make_view, scenes, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
io_ply = importlib.import_module("3dgrut_amd.io_ply")
native = importlib.import_module("3dgrut_amd.native")
surface = importlib.import_module("3dgrut_amd.surface")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
_capi = importlib.import_module("3dgrut_amd._capi")
DEV = "cuda:0"
NAME = "gut_trace_surface"
MODES = tuple(("level", lv) for lv in sr.LEVELS) + (("max_weight", 0.5),)


def _device_view(view):
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def _raster(conf=None):
    return gut.Tracer({"render": dict(conf or {})}).tracer_wrapper


def _forward(raster, d12, sph, v):
    return raster.trace(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"])


def _surface(raster, d12, v, mode="level", level=0.5, with_id=True, with_weight=True, out=None):
    return raster.trace_surface(0, 3, d12, v["ro"], v["rd"], *v["tail"], mode=mode, level=level, with_id=with_id, with_weight=with_weight,
                                out=out)


def _case_on_device(name):
    case = cr.case(name)
    raster = _raster(case["conf"])
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    return case, raster, v, d12, sph


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name", cr.CASES)
def test_planes_against_the_reference(name, max_near=0.05):
    """Both modes, the levels 0.5, 0.1 and 0.9.  A pixel is NEAR where another valid fp32 evaluation may choose differently: in
    level mode where some accepted entry has |T_after - level| <= slack(p), in largest-weight mode where the two largest reference
    weights differ by at most 2 slack(p), slack(p) = COLOUR_TOL + PIX_FLIP x the pixel's flip budget.  A pixel that is not near has
    exactly the reference's id (or none), its distance within COLOUR_TOL relative to max(1, largest reference distance) and, in
    largest-weight mode, its weight within slack(p).  A near pixel still has an id from its reference list, or none.  The near set
    is at most 5 % of the pixels that composited anything (tests/test_cpu_surface.py)."""
    case, raster, v, d12, sph = _case_on_device(name)
    s = sr.surface_case(name)
    H, W = case["H"], case["W"]
    _forward(raster, d12, sph, v)
    for mode, level in MODES:
        ref = sr.level_planes(name, level) if mode == "level" else sr.max_weight_planes(name)
        dist, ids, wgt = _surface(raster, d12, v, mode, level)
        torch.cuda.synchronize()
        assert dist.dtype == torch.float32 and ids.dtype == torch.int64 and wgt.dtype == torch.float32
        assert tuple(dist.shape) == tuple(ids.shape) == tuple(wgt.shape) == (H, W)
        dist, ids, wgt = dist.cpu().numpy().astype(np.float64), ids.cpu().numpy(), wgt.cpu().numpy().astype(np.float64)
        near = ref["near"]
        calm = ~near
        far = max(1.0, float(ref["distance"].max()))
        wrong_id = (ids != ref["id"]) & calm
        dist_err = np.abs(dist - ref["distance"]) / far
        w_err = np.abs(wgt - ref["weight"])
        print(f"[surface {name} {mode} {level}] {int(near.sum())} near of {int(s['hit'].sum())} pixels with a hit; not near: {int(wrong_id.sum())} ids "
              f"differ, worst distance difference {float(dist_err[calm].max()):.3e} (COLOUR_TOL {COLOUR_TOL:.0e}), worst weight difference / slack "
              f"{float((w_err / s['slack'])[calm].max()):.3e}; near: {int(((ids != ref['id']) & near).sum())} ids differ; {int((ids >= 0).sum())} ids")
        assert near.sum() <= max_near * s["hit"].sum()
        assert not wrong_id.any()
        assert bool((dist_err[calm] <= COLOUR_TOL).all())
        if mode == "max_weight":
            assert bool((w_err[calm] <= s["slack"][calm]).all())
        for py, px in zip(*np.nonzero(near)):
            assert ids[py, px] == -1 or ids[py, px] in s["entries"][py * W + px][0], (py, px)
        # the three planes say the same thing about which pixels have a surface
        assert np.array_equal(ids >= 0, dist > 0) and np.array_equal(ids >= 0, wgt > 0)
        if not (cr.base_name(name) == "single_tile_1025" and mode == "level" and level == 0.1):
            assert int((ids >= 0).sum()) > 0
        else:
            assert not (ids >= 0).any() and not dist.any() and not wgt.any()          # nothing crosses: the all-none plane


@pytest.mark.parametrize("name", ["ragged_70x45", "fisheye", "single_tile_1025"])
def test_exact_properties(name):
    """Per mode: two calls give identical bytes; sentinel-filled planes are overwritten in full; without the id and weight planes
    the distance bytes are the same."""
    case, raster, v, d12, sph = _case_on_device(name)
    H, W = case["H"], case["W"]
    rgba, dist_f, hits, vis = _forward(raster, d12, sph, v)
    for mode, level in (("level", 0.5), ("level", 0.9), ("max_weight", 0.5)):
        a, b = _surface(raster, d12, v, mode, level), _surface(raster, d12, v, mode, level)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))
        assert bool((a[1] >= 0).any())
        out = (torch.full((H, W), 12345.0, device=DEV), torch.full((H, W), 12345, dtype=torch.int32, device=DEV), torch.full((H, W), 12345.0, device=DEV))
        got = _surface(raster, d12, v, mode, level, out=out)
        assert got[0] is out[0] and got[2] is out[2]
        assert torch.equal(_bits(out[0]), _bits(a[0])) and torch.equal(out[1].to(torch.int64), a[1]) and torch.equal(_bits(out[2]), _bits(a[2]))
        alone = _surface(raster, d12, v, mode, level, with_id=False, with_weight=False)
        assert alone[1] is None and alone[2] is None and torch.equal(_bits(alone[0]), _bits(a[0]))
        only_id = _surface(raster, d12, v, mode, level, with_id=True, with_weight=False)
        assert only_id[2] is None and torch.equal(only_id[1], a[1]) and torch.equal(_bits(only_id[0]), _bits(a[0]))
        no_hit = hits.reshape(H, W) == 0
        assert bool((a[1][no_hit] == -1).all()) and not bool(a[0][no_hit].any()) and not bool(a[2][no_hit].any())
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", cr.CASES)
def test_level_mode_against_the_forwards_alpha(name):
    """A pixel has an id iff its final |T| < level, and the forward's alpha is 1 - T of the same products: alpha > 1 - level + 2^-23
    implies an id, alpha < 1 - level - 2^-23 none; a pixel without a hit has none."""
    case, raster, v, d12, sph = _case_on_device(name)
    H, W = case["H"], case["W"]
    rgba, dist_f, hits, vis = _forward(raster, d12, sph, v)
    alpha = rgba.reshape(H, W, 4)[..., 3].double()
    for level in sr.LEVELS:
        _, ids, _ = _surface(raster, d12, v, "level", level)
        has = ids >= 0
        above, below = alpha > 1.0 - level + 2.0 ** -23, alpha < 1.0 - level - 2.0 ** -23
        print(f"[surface vs alpha {name} {level}] {int(has.sum())} ids, {int(above.sum())} pixels above, {int(below.sum())} below, "
              f"{int((~above & ~below).sum())} within 2^-23")
        assert bool(has[above].all()) and not bool(has[below].any())
        assert not bool(has[hits.reshape(H, W) == 0].any())
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", cr.CASES)
def test_largest_weight_mode_against_the_contribution_records(name):
    """The weight plane holds the very w gut_trace_contribution takes the maximum of: for every Gaussian the largest weight(p) over
    the pixels with id(p) = i is at most the record's max_weight, as float bits, and the largest value of the plane equals the
    largest max_weight of all records bit for bit."""
    case, raster, v, d12, sph = _case_on_device(name)
    n = case["d12"].shape[0]
    _forward(raster, d12, sph, v)
    _, ids, wgt = _surface(raster, d12, v, "max_weight")
    scores = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores)
    torch.cuda.synchronize()
    record_bits = scores[:, 1] & 0xFFFFFFFF                         # the low word: the float bits of the largest weight
    has = ids >= 0
    plane_bits = _bits(wgt).to(torch.int64)[has]                    # non-negative floats order as their bits
    per_row = torch.zeros((n,), dtype=torch.int64, device=DEV).scatter_reduce_(0, ids[has], plane_bits, reduce="amax")
    assert bool((per_row <= record_bits).all())
    assert int(plane_bits.max()) == int(record_bits.max()) and int(plane_bits.max()) > 0
    # a Gaussian that holds some pixel's largest weight holds its own largest weight there or elsewhere: rows that are some pixel's
    # choice were composited
    assert bool((record_bits[ids[has]] > 0).all())


def test_nothing_else_changes():
    """With and without surface calls between the forward and what follows it: the forward outputs, the gradient rows, the records
    of a following contribution call, the planes of a following attribute call and the lists and depths the backward reads are the
    same, bit for bit.  The gradients of the following backward are compared bit for bit WHERE THAT SAYS SOMETHING: the backward
    compositor adds into the gradient rows with float atomics, whose arrival order is not fixed, so two runs WITHOUT a surface call
    are the control.  Where the control pair is bit-identical, the pair with and without must be; where it is not, the gradients
    after the call are held to the oracle's backward by the project's own row bar.  Both comparisons are printed."""
    from tests.common import ROW_FLIP_BOUND, check_gradients_per_row
    oracle = importlib.import_module("oracle.oracle")
    case = cr.case("pinhole_64x48")
    n, W, H = 300, case["W"], case["H"]
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    attrs = torch.as_tensor(np.random.default_rng(9).uniform(-1, 1, (n, 5)).astype(np.float32), device=DEV)
    rgba_grad_host = np.random.default_rng(11).normal(size=(H, W, 4)).astype(np.float32)
    rgba_grad = torch.as_tensor(rgba_grad_host, device=DEV)
    lists = ("ordered_ids", "tile_ranges", "tile_traversed_fwd")

    def run(with_surface):
        raster = _raster()
        outs = _forward(raster, d12, sph, v)
        raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.ones_like(outs[0]), outs[1], None)
        outs = _forward(raster, d12, sph, v)
        before = [o.clone() for o in outs]
        if with_surface:
            _surface(raster, d12, v, "level", 0.5)
            _surface(raster, d12, v, "max_weight")
            _surface(raster, d12, v, "level", 0.9, with_id=False, with_weight=False)
        for o, b in zip(outs, before):
            assert torch.equal(o, b)
        scratch = raster.debug_buffer("grad_scratch").clone()
        read = [raster.debug_buffer(k).clone() for k in lists]
        scores = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
        raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores)
        planes = raster.trace_attributes(0, 3, d12, attrs, v["ro"], v["rd"], *v["tail"])
        g12, g48 = raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], rgba_grad, outs[1], None)
        torch.cuda.synchronize()
        return [o.clone() for o in outs], scratch, scores, g12.clone(), g48.clone(), read, planes.clone()

    plain, control, touched = run(False), run(False), run(True)
    for o, b in zip(plain[0], touched[0]):
        assert torch.equal(o, b)
    assert torch.equal(plain[1], touched[1]) and not bool(touched[1].any())
    assert torch.equal(plain[2], touched[2]) and bool(plain[2].any())
    assert torch.equal(_bits(plain[6]), _bits(touched[6])) and bool(plain[6].any())
    for k, a, b in zip(lists, plain[5], touched[5]):
        assert torch.equal(a, b), k
    assert tuple(plain[3].shape) == (n, 12) and tuple(plain[4].shape) == (n, 48) and bool(plain[3].any()) and bool(plain[4].any())
    same = lambda x, y: torch.equal(_bits(x[3]), _bits(y[3])) and torch.equal(_bits(x[4]), _bits(y[4]))
    worst = lambda x, y: max(float((x[3] - y[3]).abs().max()), float((x[4] - y[4]).abs().max()))
    print(f"[surface disturbs nothing] gradients of two runs without the call bit-identical: {same(plain, control)} (largest difference "
          f"{worst(plain, control):.3e}); with and without the call: {same(plain, touched)} (largest difference {worst(plain, touched):.3e})")
    if same(plain, control):
        assert same(plain, touched)
    dens_g, sph_g, _, budget = oracle.backward(case["view"]["oracle_cam"], case["ref"], rgba_grad_host, np.zeros((H, W, 1), np.float32),
                                               flip_bound=ROW_FLIP_BOUND)
    check_gradients_per_row(touched[3].cpu().numpy(), touched[4].cpu().numpy(), dens_g, sph_g, "backward after trace_surface", budget=budget)


def _raw_call(raster, n, d12, v, mode, level, dist_ptr, id_ptr, weight_ptr, stream=None):
    cam = raster._camera(*v["tail"])
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    H, W = int(v["ro"].shape[1]), int(v["ro"].shape[2])
    return raster._lib.gut_trace_surface(raster._handle, C.c_void_p(st), 0, 3, n, d12.data_ptr(), W, H, v["ro"].data_ptr(), v["rd"].data_ptr(),
                                         C.byref(cam), mode, level, dist_ptr, id_ptr, weight_ptr)


def test_refusals_leave_the_handle_rendering():
    case, other = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n, H, W = 300, case["H"], case["W"]
    v, vo = _device_view(case["view"]), _device_view(other["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    raster = _raster()
    out = (torch.zeros((H, W), device=DEV), torch.zeros((H, W), dtype=torch.int32, device=DEV), torch.zeros((H, W), device=DEV))
    dp, ip, wp = (t.data_ptr() for t in out)

    def refused(pattern, call, error=RuntimeError):
        with pytest.raises(error, match=pattern):
            call()
        torch.cuda.synchronize()
        assert not any(bool(t.any()) for t in out), f"{pattern!r}: the refused call wrote"

    def raw(*a, **kw):
        _capi.check(_raw_call(raster, *a, **kw), "trace_surface")

    LEVEL, MAXW = _capi.SURFACE_LEVEL, _capi.SURFACE_MAX_WEIGHT
    refused(re.escape(f"{NAME}: no forward context on this stream"), lambda: _surface(raster, d12, v, out=out))
    ref_out = [o.clone() for o in _forward(raster, d12, sph, v)]
    side = torch.cuda.Stream(DEV)
    refused(re.escape(f"{NAME}: no forward context on this stream"), lambda: raw(n, d12, v, LEVEL, 0.5, dp, ip, wp, stream=side.cuda_stream))
    refused(re.escape(f"{NAME}: camera differs from the cached forward"),
            lambda: raster.trace_surface(0, 3, d12, v["ro"], v["rd"], *vo["tail"], with_weight=True, out=out))
    refused(re.escape(f"{NAME}: arguments differ from the cached forward"), lambda: raw(n - 1, d12, v, LEVEL, 0.5, dp, ip, wp))
    for bad_mode in (2, -1):
        refused(re.escape(f"{NAME}: mode must be GUT_SURFACE_LEVEL (0) or GUT_SURFACE_MAX_WEIGHT (1), got {bad_mode}"),
                lambda: raw(n, d12, v, bad_mode, 0.5, dp, ip, wp))
    # the level: finite and inside (min_transmittance, 1); the default min_transmittance is 1e-4
    for bad_level in (float("nan"), float("inf"), 1.0, 1.5, 0.0, -0.5, 1e-4, 5e-5):
        refused(re.escape(f"{NAME}: level must be finite and inside (min_transmittance, 1)"), lambda: raw(n, d12, v, LEVEL, bad_level, dp, ip, wp))
        refused(re.escape(f"{NAME}: level must be finite and inside (min_transmittance, 1)"),
                lambda: _surface(raster, d12, v, "level", bad_level, out=out))
    refused(re.escape(f"{NAME}: d_distance is NULL"), lambda: raw(n, d12, v, LEVEL, 0.5, None, ip, wp))
    refused(re.escape(f"{NAME}: d_distance is NULL"), lambda: raw(n, d12, v, MAXW, 0.5, None, None, None))
    refused(re.escape(f"{NAME}: d_distance must be 4-byte aligned"), lambda: raw(n, d12, v, LEVEL, 0.5, dp + 2, ip, wp))
    refused(re.escape(f"{NAME}: d_id must be 4-byte aligned"), lambda: raw(n, d12, v, LEVEL, 0.5, dp, ip + 1, wp))
    refused(re.escape(f"{NAME}: d_weight must be 4-byte aligned"), lambda: raw(n, d12, v, MAXW, 0.5, dp, ip, wp + 2))
    # the Python surface checks its mode and its tensors before the library sees them
    refused("surface mode: one of", lambda: _surface(raster, d12, v, "median", out=out))
    refused("surface mode: one of", lambda: _surface(raster, d12, v, 0, out=out))
    f32, i32 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.int32, device=DEV)
    for bad_dist in (torch.zeros((W, H), **f32), torch.zeros((H, W), dtype=torch.float64, device=DEV), torch.zeros((H, W)),
                     torch.zeros((H, 2 * W), **f32)[:, ::2], None):
        refused("surface distance: a contiguous float32 tensor", lambda: _surface(raster, d12, v, out=(bad_dist, out[1], out[2])))
    for bad_id in (torch.zeros((H, W), dtype=torch.int64, device=DEV), torch.zeros((H, W), **f32), torch.zeros((H + 1, W), **i32),
                   torch.zeros((H, W), dtype=torch.int32)):
        refused("surface id: a contiguous int32 tensor", lambda: _surface(raster, d12, v, out=(out[0], bad_id, out[2])))
    for bad_w in (torch.zeros((H, W), **i32), torch.zeros((1, H, W), **f32), torch.zeros((H, W))):
        refused("surface weight: a contiguous float32 tensor", lambda: _surface(raster, d12, v, out=(out[0], out[1], bad_w)))
    refused("id and weight tensors exactly where", lambda: _surface(raster, d12, v, with_weight=False, out=out))
    refused("id and weight tensors exactly where", lambda: _surface(raster, d12, v, out=(out[0], None, out[2])))
    refused(r"a \(distance, id, weight\) triple", lambda: _surface(raster, d12, v, out=out[0]))
    refused("rayOrigin", lambda: raster.trace_surface(0, 3, d12, v["ro"].double(), v["rd"], *v["tail"], with_weight=True, out=out))
    refused("particleDensity", lambda: raster.trace_surface(0, 3, d12[:, :11], v["ro"], v["rd"], *v["tail"], with_weight=True, out=out))
    # the handle still renders as an untouched one
    got = _surface(raster, d12, v)
    fresh = _raster()
    _forward(fresh, d12, sph, v)
    want = _surface(fresh, d12, v)
    again = _forward(raster, d12, sph, v)
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and bool((got[1] >= 0).any())
    for o, b in zip(again, ref_out):
        assert torch.equal(o, b)

    for conf, what in (({"splat": {"k_buffer_size": 16}}, "k_buffer_size=16"), ({"particle_kernel_degree": 4}, "particle_kernel_degree=4")):
        r = _raster(conf)
        outs = [o.clone() for o in _forward(r, d12, sph, v)]
        with pytest.raises(RuntimeError, match=re.escape(f"{NAME}: supported on the unsorted variant (k_buffer_size=0) at particle_kernel_degree=2 only") + ".*" + re.escape(what)):
            _surface(r, d12, v, out=out)
        torch.cuda.synchronize()
        assert not any(bool(t.any()) for t in out)
        for o, b in zip(_forward(r, d12, sph, v), outs):
            assert torch.equal(o, b)


def test_a_call_after_the_early_optimiser_pass_is_refused():
    sc = scenes.scene_c1(300, 0)
    view = make_view("pinhole", 64, 48, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)), fx=64.0)
    batch = to_batch(view, DEV)
    st = native.NativeTrainStep(native.NativeGaussianModel(sc, device=DEV), gut.Tracer({"render": {}}), overlap_optimizer=True)
    st.lr12[:] = 0.0
    st.lr48[:] = 0.0
    st.forward(batch)
    _, sensor, poses, _, _ = st._ctx
    tail = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
    out = (torch.zeros((48, 64), device=DEV), torch.zeros((48, 64), dtype=torch.int32, device=DEV), None)
    args = (0, 3, st.act, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(), *tail)
    st.raster.optimize_rows_without_gradient(*st._state(), *st._adam_settings(), st.act, lazy=st._lazy())
    with pytest.raises(RuntimeError, match=f"{NAME}: gut_optimize_rows_without_gradient was called for this forward"):
        st.raster.trace_surface(*args, out=out)
    torch.cuda.synchronize()
    assert not bool(out[0].any()) and not bool(out[1].any())
    st.raster.finish_optimizer_step_without_gradient()                   # ends the half-applied step; then the handle goes on
    st.forward(batch)
    st.raster.trace_surface(*args, out=out)
    torch.cuda.synchronize()
    assert bool(out[0].any()) and bool((out[1] >= 0).any())


def test_empty_inputs_give_the_no_hit_planes():
    case = cr.case("pinhole_64x48")
    H, W = case["H"], case["W"]
    v = _device_view(case["view"])
    raster = _raster()

    def check(d12, view):
        for mode in ("level", "max_weight"):
            out = (torch.full((H, W), 7.0, device=DEV), torch.full((H, W), 7, dtype=torch.int32, device=DEV), torch.full((H, W), 7.0, device=DEV))
            dist, ids, wgt = _surface(raster, d12, view, mode, out=out)
            torch.cuda.synchronize()
            assert not bool(out[0].any()) and not bool(out[2].any()) and bool((out[1] == -1).all()) and bool((ids == -1).all())
            alone = torch.full((H, W), 7.0, device=DEV)
            _surface(raster, d12, view, mode, with_id=False, with_weight=False, out=(alone, None, None))
            torch.cuda.synchronize()
            assert not bool(alone.any())

    # no Gaussians
    d12, sph = torch.zeros((0, 12), device=DEV), torch.zeros((0, 48), device=DEV)
    _forward(raster, d12, sph, v)
    check(d12, v)
    # a view that sees nothing: the scene lies behind the camera
    away = _device_view(make_view("pinhole", W, H, cams.look_at_c2w((0.3, -0.2, -4.0), (0.6, -0.4, -8.0)), fx=64.0))
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    _forward(raster, d12, sph, away)
    assert raster.stats()["num_intersections"] == 0
    check(d12, away)


def test_backproject_on_the_device():
    """surface.backproject on the reference distances against the float64 c2w arithmetic: 1e-5 relative to the largest coordinate,
    a float32 matrix-vector product's bar; a distance of 0 gives NaN."""
    s = sr.surface_case("ragged_70x45")
    dist = sr.level_planes("ragged_70x45", 0.5)["distance"]
    want = sr.backproject(s["view"], dist)
    got = surface.backproject(to_batch(s["view"], DEV), torch.as_tensor(dist, device=DEV))
    assert got.is_cuda and tuple(got.shape) == (s["H"], s["W"], 3) and got.dtype == torch.float32
    got = got.cpu().numpy()
    some = dist > 0
    assert bool(np.isnan(got[~some]).all())
    worst = float(np.abs(got[some] - want[some]).max() / np.abs(want[some]).max())
    print(f"[surface backproject on the device] worst relative difference {worst:.3e}")
    assert worst <= 1e-5


def test_the_walls_points_lie_on_the_wall():
    """fuse_points over the three wall views: every point within the reference's largest |z| plus COLOUR_TOL x the largest
    distance of the wall; SurfaceRenderer.render's dict; voxel > 0 returns a subset with one point per cell, the first of each;
    the same call twice gives the same bytes; stride takes every stride-th pixel."""
    ref = sr.wall_points()
    model = native.NativeGaussianModel(sr.wall_scene(), device=DEV)
    renderer = surface.SurfaceRenderer(model, gut.Tracer({"render": {}}))
    batches = [to_batch(view, DEV) for view in sr.wall_views()]
    W, H = sr.WALL_SIZE
    r = renderer.render(batches[1])
    assert sorted(r) == ["distance", "id", "rgba", "weight"] and tuple(r["distance"].shape) == (H, W) and r["id"].dtype == torch.int64
    assert tuple(r["rgba"].shape)[-1] == 4 and bool((r["id"] >= 0).any()) and int(r["id"].max()) < 252
    top = renderer.render(batches[1], mode="max_weight")
    assert bool(((top["id"] >= 0) | (r["id"] < 0)).all()) and bool((top["weight"] >= r["weight"]).all())
    xyz, rgb, ids = surface.fuse_points(renderer, batches)
    again = surface.fuse_points(renderer, batches)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
               for a, b in zip((xyz, rgb, ids), again))
    p = int(xyz.shape[0])
    assert tuple(xyz.shape) == (p, 3) and tuple(rgb.shape) == (p, 3) and tuple(ids.shape) == (p,) and xyz.is_cuda
    assert xyz.dtype == torch.float32 and rgb.dtype == torch.float32 and ids.dtype == torch.int64
    bound = ref["max_abs_z"] + COLOUR_TOL * ref["max_distance"]
    worst = float(xyz[:, 2].abs().max())
    print(f"[surface wall on the device] {p} points (the reference: {ref['points'].shape[0]}), largest |z| {worst:.6f}, bound {bound:.6f}")
    assert bool(torch.isfinite(xyz).all()) and worst <= bound
    assert p > 0
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0 and int(ids.min()) >= 0 and int(ids.max()) < 252
    # the Gaussian of a point is near it: within its 3 sigma radius in the plane
    centre = torch.as_tensor(sr.wall_scene()["positions"], device=DEV)[ids]
    assert float((xyz - centre).norm(dim=1).max()) <= 3.0 * 0.2 + 1e-3
    # one point per occupied cell, the first of each
    voxel = 0.1
    vx, vrgb, vid = surface.fuse_points(renderer, batches, voxel=voxel)
    cells = torch.floor(xyz.double() / voxel).to(torch.int64)
    vcells = torch.floor(vx.double() / voxel).to(torch.int64)
    assert 0 < vx.shape[0] < p and torch.unique(vcells, dim=0).shape[0] == vx.shape[0] == torch.unique(cells, dim=0).shape[0]
    first = surface.first_per_voxel(xyz, voxel)
    assert torch.equal(_bits(vx), _bits(xyz[first])) and torch.equal(_bits(vrgb), _bits(rgb[first])) and torch.equal(vid, ids[first])
    seen = {}
    for i, c in enumerate(map(tuple, cells.cpu().tolist())):
        seen.setdefault(c, i)
    assert sorted(seen.values()) == first.cpu().tolist()
    # every second pixel
    sx, _, sid = surface.fuse_points(renderer, batches[:1], stride=2)
    one = renderer.render(batches[0])
    pts = surface.backproject(batches[0], one["distance"])[::2, ::2].reshape(-1, 3)
    keep = (one["id"][::2, ::2] >= 0).reshape(-1)
    assert torch.equal(_bits(sx), _bits(pts[keep])) and torch.equal(sid, one["id"][::2, ::2].reshape(-1)[keep]) and sx.shape[0] > 0
    with pytest.raises(ValueError):
        surface.fuse_points(renderer, batches, stride=0)
    with pytest.raises(ValueError):
        surface.fuse_points(renderer, batches, voxel=-1.0)


def test_trainer_exports_points(tmp_path, capsys):
    """--export-points on a small synthetic COLMAP scene: 8 views of 96 x 96 (7 to train on, 1 held out), 40 iterations."""
    from tests.synthetic_colmap import write_synthetic_colmap
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=8, size=96, n_teacher=20_000, n_points=2_000)
    out = str(tmp_path / "run")
    assert trainer_mod.main(["--path", root, "--n-iterations", "40", "--out-dir", out, "--export-points", "--points-stride", "2"]) == 0
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    print(f"[trainer points] {stats['points_n']} points from {stats['points_views']} views at level {stats['points_level']}")
    assert stats["points_views"] == 7 and stats["points_level"] == 0.5 and 0 < stats["points_n"] <= 7 * 48 * 48
    cloud = io_ply.read_ply(os.path.join(out, "points.ply"))
    assert cloud["positions"].shape == (stats["points_n"], 3) and cloud["rgb"].shape == (stats["points_n"], 3)
    assert np.isfinite(cloud["positions"]).all()
    renders = sorted(os.listdir(os.path.join(out, "renders_depth")))
    assert len(renders) == 1 and renders[0].endswith(".npy")
    depth = np.load(os.path.join(out, "renders_depth", renders[0]))
    assert depth.dtype == np.float32 and depth.shape == (96, 96) and np.isfinite(depth).all() and depth.min() >= 0.0 and depth.max() > 0.0
    # without the flag: none of the keys, none of the files
    out2 = str(tmp_path / "plain")
    assert trainer_mod.main(["--path", root, "--n-iterations", "5", "--out-dir", out2]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    assert not any(k.startswith("points") for k in plain)
    assert not os.path.exists(os.path.join(out2, "points.ply")) and not os.path.exists(os.path.join(out2, "renders_depth"))
