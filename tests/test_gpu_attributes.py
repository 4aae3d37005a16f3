"""gut_trace_attributes on the device: the rendered attribute planes against the CPU oracle
(tests/attribute_reference.py, asserted by tests/test_cpu_attributes.py), against the device's own forward and, as the adjoint,
against gut_trace_contribution_weighted; the properties that hold exactly; that it disturbs nothing; its refusals; empty inputs; the
selection from masks end to end and through the trainer's command line."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import attribute_reference as ar
from tests import contribution_reference as cr
from tests import weighted_contribution_reference as wr
from tests.common import COLOUR_TOL, cams, make_view, scenes, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
attributes = importlib.import_module("3dgrut_amd.attributes")
io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
io_ply = importlib.import_module("3dgrut_amd.io_ply")
native = importlib.import_module("3dgrut_amd.native")
selection = importlib.import_module("3dgrut_amd.selection")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
_capi = importlib.import_module("3dgrut_amd._capi")
DEV = "cuda:0"
PAD = 0xFFFFFFFF
NAME = "gut_trace_attributes"


def _device_view(view):
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def _raster(conf=None):
    return gut.Tracer({"render": dict(conf or {})}).tracer_wrapper


def _forward(raster, d12, sph, v):
    return raster.trace(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"])


def _render(raster, d12, v, attrs, out=None):
    return raster.trace_attributes(0, 3, d12, attrs, v["ro"], v["rd"], *v["tail"], out=out)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _case_on_device(name):
    case = cr.case(name)
    raster = _raster(case["conf"])
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    return case, raster, v, d12, sph


@pytest.mark.parametrize("name", cr.CASES)
def test_planes_against_the_oracle(name):
    """K = 4 seeded attributes in [0, 1], the last channel ones: the four planes, taken as an [H,W,4] image, are held to the
    project's own image bar (common.check_colour_outliers with the per-pixel flip budget) — valid unchanged, the attributes lying
    in [0, 1] like colours."""
    from tests.common import check_colour_outliers
    case, raster, v, d12, sph = _case_on_device(name)
    a = ar.attribute_case(name)
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    out = _render(raster, d12, v, _t(a["attrs"]))
    torch.cuda.synchronize()
    H, W = case["H"], case["W"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, H, W)
    fake_ref = dict(rgba=np.ascontiguousarray(a["planes"].transpose(1, 2, 0)), hits=case["ref"]["hits"])
    check_colour_outliers(out.permute(1, 2, 0).cpu().numpy(), hits.cpu().numpy(), fake_ref, a["margins"], label=f"attributes {name}",
                          budget=a["budget"])
    assert float(out.max()) > 0.05


@pytest.mark.parametrize("name", cr.CASES)
def test_planes_against_the_devices_own_forward(name):
    """Channels = the colours the forward composited (max(feat, 0), the handle's per-view colour buffer) and ones, against the
    forward's rgba.  The weights are the forward's bits; a colour is at most hits(p) fused multiply-adds on partial sums <= 1, each
    rounding by <= 2^-24, and the forward's own accumulation gives the same again: |difference| <= (hits(p) + 2) * 2^-23 per pixel.
    The forward forms its alpha as 1 - T, a product of the factors (1 - alpha_i), not as a sum of weights: that channel is held to
    COLOUR_TOL instead."""
    case, raster, v, d12, sph = _case_on_device(name)
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    feat = raster.debug_buffer("feat")[:3 * n].reshape(n, 3)
    attrs = torch.cat([feat.clamp_min(0.0), torch.ones((n, 1), device=DEV)], dim=1).contiguous()
    out = _render(raster, d12, v, attrs)
    torch.cuda.synchronize()
    diff = (out.permute(1, 2, 0).double() - rgba.reshape(H, W, 4).double()).abs()
    bound = (hits.reshape(H, W).double() + 2.0) * 2.0 ** -23
    ratio = float((diff[..., :3].amax(-1) / bound).max())
    print(f"[attributes vs forward {name}] colours: largest difference / bound {ratio:.3f} (largest difference {float(diff[..., :3].max()):.3e}); "
          f"alpha: largest difference {float(diff[..., 3].max()):.3e} (COLOUR_TOL {COLOUR_TOL:.0e})")
    assert bool((diff[..., :3].amax(-1) <= bound).all())
    assert float(diff[..., 3].max()) <= COLOUR_TOL
    assert float(out[:3].max()) > 0.01


@pytest.mark.parametrize("name", cr.CASES)
def test_adjoint_of_the_weighted_contribution_walk(name):
    """Seeded P in [0, 1] and one signed channel a in [-1, 1]:  | sum_p P out - sum_i a_i weighted_i 2^-32 | <= 2^-20 sum_p (hits(p) + 2),
    both sides summed in float64 on the host.  Both sum the same products w a P from bit-identical w; 2^-20 is eight half-ulps per
    composited term and covers the fp32 accumulation here, the DPP tree and wave combination there, and the q32 rounding."""
    case, raster, v, d12, sph = _case_on_device(name)
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    plane = _t(wr.weighted_case(name)["plane"])
    a = torch.as_tensor(np.random.default_rng(90 + cr.case_index(name)).uniform(-1, 1, n).astype(np.float32), device=DEV)
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    out = _render(raster, d12, v, a[:, None].contiguous())
    wq = torch.zeros((n,), dtype=torch.int64, device=DEV)
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], None, pixel_weight=plane, weighted=wq)
    torch.cuda.synchronize()
    lhs = float((plane.double() * out[0].double()).sum())
    rhs = float((a.double() * wq.double() * 2.0 ** -32).sum())
    bound = 2.0 ** -20 * float((hits.double() + 2.0).sum())
    print(f"[attributes adjoint {name}] sum P out {lhs!r} vs sum a weighted {rhs!r}: difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert bool(wq.any()) and bool((out != 0).any()) and float(out.min()) < 0 < float(out.max())


def test_channel_counts():
    """K = 1, 3, 4, 5 and 9 on the ragged case: channel k of every K is the K = 1 render of that column, bit for bit (one walk per
    group of four, a last group of one or three channels, the 16-byte and the 4-byte gather); a 1-D [N] input is [N,1]; rows that
    do not start on 16-byte boundaries give the bits of their aligned copy."""
    case, raster, v, d12, sph = _case_on_device("ragged_70x45")
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    cols = _t(np.random.default_rng(7).uniform(-1, 1, (n, 9)))
    _forward(raster, d12, sph, v)
    single = [_render(raster, d12, v, cols[:, k:k + 1].contiguous())[0] for k in range(9)]
    for k_total in (1, 3, 4, 5, 9):
        out = _render(raster, d12, v, cols[:, :k_total].contiguous())
        assert tuple(out.shape) == (k_total, H, W)
        for k in range(k_total):
            assert torch.equal(out[k], single[k]), (k_total, k)
    assert all(bool(s.any()) for s in single) and not torch.equal(single[0], single[1])
    # 1-D through the renderer
    model = native.NativeGaussianModel(scenes.scene_c1(333, 0), device=DEV)
    renderer = attributes.AttributeRenderer(model, gut.Tracer({"render": {}}))
    batch = to_batch(case["view"], DEV)
    one, two = renderer.render(batch, cols[:, 0]), renderer.render(batch, cols[:, :1])
    assert tuple(one.shape) == (1, H, W) and torch.equal(one, two) and bool(one.any())
    flags = renderer.render(batch, cols[:, 0] > 0)
    assert torch.equal(flags, renderer.render(batch, (cols[:, 0] > 0).float()))
    rgba, both = renderer.render_with_image(batch, cols[:, :2])
    assert tuple(rgba.shape)[-1] == 4 and torch.equal(both[:1], one)
    # [N,8] rows offset by one float: 4-byte loads; the aligned copy takes the 16-byte ones
    store = torch.zeros(n * 8 + 4, dtype=torch.float32, device=DEV)
    shifted = store[1:1 + n * 8].view(n, 8)
    shifted.copy_(cols[:, :8])
    aligned = cols[:, :8].contiguous()
    assert shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and shifted.is_contiguous()
    _forward(raster, d12, sph, v)
    assert torch.equal(_render(raster, d12, v, shifted), _render(raster, d12, v, aligned))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["ragged_70x45", "fisheye", "single_tile_1025"])
def test_exact_properties(name):
    """Two calls give identical bytes; negated attributes give the negated planes; a pre-filled output is overwritten in full;
    pixels without a hit are exactly 0; NaN attributes on Gaussians the forward did not walk (the fisheye case has one, the
    single-tile case thousands without a tile; the ragged case none) leave every pixel as it was."""
    case, raster, v, d12, sph = _case_on_device(name)
    ref, n, H, W = case["ref"], case["d12"].shape[0], case["H"], case["W"]
    attrs = _t(np.random.default_rng(8).uniform(-1, 1, (n, 5)))
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    a, b = _render(raster, d12, v, attrs), _render(raster, d12, v, attrs)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(a.any())                 # identical bytes
    neg = _render(raster, d12, v, -attrs)
    assert torch.equal(neg, -a)
    nz = a != 0
    assert torch.equal(neg.view(torch.int32)[nz], (-a).view(torch.int32)[nz])                      # bit for bit where not zero
    sentinel = torch.full((5, H, W), 12345.0, dtype=torch.float32, device=DEV)
    assert _render(raster, d12, v, attrs, out=sentinel) is sentinel
    assert torch.equal(sentinel, a)                                                                # fully overwritten
    no_hit = (hits.reshape(H, W) == 0)
    assert not bool(a[:, no_hit].any())
    assert torch.equal(a.view(torch.int32)[:, no_hit], torch.zeros_like(a.view(torch.int32)[:, no_hit]))
    if cr.base_name(name) == "ragged_70x45":
        assert int(no_hit.sum()) > 0
    # a NaN on Gaussians the forward did not walk reaches no pixel
    ordered = raster.debug_buffer("ordered_ids").cpu().numpy().view(np.uint32)
    trav = raster.debug_buffer("tile_traversed_fwd").cpu().numpy().view(np.uint32)
    walked = np.zeros(n, bool)
    for t, (b0, e0) in enumerate(ref["tile_ranges"]):
        ids = ordered[b0:b0 + min(int(trav[t]), int(e0) - int(b0))]
        walked[ids[ids != PAD]] = True
    unwalked = ~walked | (ref["tiles_count"] == 0)
    assert (int(unwalked.sum()) > 0) == (cr.base_name(name) != "ragged_70x45")
    poisoned = attrs.clone()
    poisoned[torch.as_tensor(unwalked, device=DEV)] = float("nan")
    got = _render(raster, d12, v, poisoned)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, a)
    print(f"[attributes exact {name}] {int(unwalked.sum())} of {n} rows unwalked and poisoned, {int(no_hit.sum())} pixels without a hit")


def test_nothing_else_changes():
    """With and without attribute calls between the forward and what follows it: the four forward outputs, the gradient rows and
    the records of a following contribution call are the same, bit for bit, and so are the lists and depths the backward reads.
    The gradients of the following backward are compared bit for bit too WHERE THAT SAYS SOMETHING: the backward compositor adds
    into the gradient rows with float atomics, whose arrival order is not fixed, so two runs WITHOUT an attribute
    call are the control.  Where the control pair is bit-identical, the pair with and without must be; where it is not, bits say
    nothing about the call, and the gradients after it are held to the oracle's backward by the project's own row bar
    (common.check_gradients_per_row), as the contribution tests hold theirs.  Both comparisons are printed."""
    from tests.common import ROW_FLIP_BOUND, check_gradients_per_row
    oracle = importlib.import_module("oracle.oracle")
    case = cr.case("pinhole_64x48")
    n, W, H = 300, case["W"], case["H"]
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    attrs = _t(np.random.default_rng(9).uniform(-1, 1, (n, 6)))
    rgba_grad_host = np.random.default_rng(11).normal(size=(H, W, 4)).astype(np.float32)
    rgba_grad = torch.as_tensor(rgba_grad_host, device=DEV)
    lists = ("ordered_ids", "tile_ranges", "tile_traversed_fwd")

    def run(with_attributes):
        raster = _raster()
        # (a first forward and backward, so that the handle has gradient rows to show: every consumer leaves them zero)
        outs = _forward(raster, d12, sph, v)
        raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.ones_like(outs[0]), outs[1], None)
        outs = _forward(raster, d12, sph, v)
        before = [o.clone() for o in outs]
        if with_attributes:
            _render(raster, d12, v, attrs)
            _render(raster, d12, v, attrs[:, :1].contiguous())
        for o, b in zip(outs, before):
            assert torch.equal(o, b)
        scratch = raster.debug_buffer("grad_scratch").clone()
        read = [raster.debug_buffer(k).clone() for k in lists]
        scores = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
        raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores)
        g12, g48 = raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], rgba_grad, outs[1], None)
        torch.cuda.synchronize()
        return [o.clone() for o in outs], scratch, scores, g12.clone(), g48.clone(), read

    plain, control, touched = run(False), run(False), run(True)
    for o, b in zip(plain[0], touched[0]):
        assert torch.equal(o, b)
    assert torch.equal(plain[1], touched[1]) and not bool(touched[1].any())
    assert torch.equal(plain[2], touched[2]) and bool(plain[2].any())
    for k, a, b in zip(lists, plain[5], touched[5]):
        assert torch.equal(a, b), k
    assert tuple(plain[3].shape) == (n, 12) and tuple(plain[4].shape) == (n, 48) and bool(plain[3].any()) and bool(plain[4].any())
    bits = lambda t: t.view(torch.int32)
    same = lambda x, y: torch.equal(bits(x[3]), bits(y[3])) and torch.equal(bits(x[4]), bits(y[4]))
    worst = lambda x, y: max(float((x[3] - y[3]).abs().max()), float((x[4] - y[4]).abs().max()))
    print(f"[attributes disturb nothing] gradients of two runs without the call bit-identical: {same(plain, control)} (largest difference "
          f"{worst(plain, control):.3e}); with and without the call: {same(plain, touched)} (largest difference {worst(plain, touched):.3e})")
    if same(plain, control):
        assert same(plain, touched)
    dens_g, sph_g, _, budget = oracle.backward(case["view"]["oracle_cam"], case["ref"], rgba_grad_host, np.zeros((H, W, 1), np.float32),
                                               flip_bound=ROW_FLIP_BOUND)
    check_gradients_per_row(touched[3].cpu().numpy(), touched[4].cpu().numpy(), dens_g, sph_g, "backward after trace_attributes", budget=budget)


def _raw_call(raster, n, d12, v, k, attrs_ptr, out_ptr, stream=None):
    cam = raster._camera(*v["tail"])
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    H, W = int(v["ro"].shape[1]), int(v["ro"].shape[2])
    return raster._lib.gut_trace_attributes(raster._handle, C.c_void_p(st), 0, 3, n, d12.data_ptr(), W, H, v["ro"].data_ptr(),
                                            v["rd"].data_ptr(), C.byref(cam), k, attrs_ptr, out_ptr)


def test_refusals_leave_the_handle_rendering():
    case, other = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n, H, W = 300, case["H"], case["W"]
    v, vo = _device_view(case["view"]), _device_view(other["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    attrs = _t(np.random.default_rng(10).uniform(0, 1, (n, 2)))
    raster = _raster()
    out = torch.zeros((2, H, W), dtype=torch.float32, device=DEV)

    def refused(pattern, call, error=RuntimeError):
        with pytest.raises(error, match=pattern):
            call()
        torch.cuda.synchronize()
        assert not bool(out.any()), f"{pattern!r}: the refused call wrote"

    def raw(*a, **kw):
        _capi.check(_raw_call(raster, *a, **kw), "trace_attributes")

    refused(re.escape(f"{NAME}: no forward context on this stream"), lambda: _render(raster, d12, v, attrs, out=out))
    ref_out = [o.clone() for o in _forward(raster, d12, sph, v)]
    side = torch.cuda.Stream(DEV)
    refused(re.escape(f"{NAME}: no forward context on this stream"),
            lambda: raw(n, d12, v, 2, attrs.data_ptr(), out.data_ptr(), stream=side.cuda_stream))
    refused(re.escape(f"{NAME}: camera differs from the cached forward"),
            lambda: raster.trace_attributes(0, 3, d12, attrs, v["ro"], v["rd"], *vo["tail"], out=out))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 0"), lambda: raw(n, d12, v, 0, attrs.data_ptr(), out.data_ptr()))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 65"), lambda: raw(n, d12, v, 65, attrs.data_ptr(), out.data_ptr()))
    refused(re.escape(f"{NAME}: d_attributes is NULL"), lambda: raw(n, d12, v, 2, None, out.data_ptr()))
    refused(re.escape(f"{NAME}: d_out is NULL"), lambda: raw(n, d12, v, 2, attrs.data_ptr(), None))
    refused(re.escape(f"{NAME}: d_out must be 4-byte aligned"), lambda: raw(n, d12, v, 2, attrs.data_ptr(), out.data_ptr() + 2))
    refused(re.escape(f"{NAME}: arguments differ from the cached forward"), lambda: raw(n - 1, d12, v, 2, attrs.data_ptr(), out.data_ptr()))
    # the Python surface checks its tensors before the library sees them
    for bad in (attrs[:n - 1], attrs[:, 0], attrs.double(), attrs.cpu(), attrs.t().contiguous().t(), attrs.to(torch.int32)):
        refused(r"attributes: a contiguous float32 tensor \[300, K\]", lambda: _render(raster, d12, v, bad, out=out))
    for bad_out in (torch.zeros((3, H, W), device=DEV), torch.zeros((2, H, W), dtype=torch.float64, device=DEV), torch.zeros((2, W, H), device=DEV)):
        refused("attribute output", lambda: _render(raster, d12, v, attrs, out=bad_out))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 0"), lambda: _render(raster, d12, v, attrs[:, :0].contiguous()))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 65"), lambda: _render(raster, d12, v, torch.zeros((n, 65), device=DEV)))
    # the handle still renders as an untouched one
    got = _render(raster, d12, v, attrs)
    fresh = _raster()
    _forward(fresh, d12, sph, v)
    want = _render(fresh, d12, v, attrs)
    again = _forward(raster, d12, sph, v)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(got.any())
    for o, b in zip(again, ref_out):
        assert torch.equal(o, b)

    for conf, what in (({"splat": {"k_buffer_size": 16}}, "k_buffer_size=16"), ({"particle_kernel_degree": 4}, "particle_kernel_degree=4")):
        r = _raster(conf)
        outs = [o.clone() for o in _forward(r, d12, sph, v)]
        with pytest.raises(RuntimeError, match=re.escape(f"{NAME}: supported on the unsorted variant (k_buffer_size=0) at particle_kernel_degree=2 only") + ".*" + re.escape(what)):
            _render(r, d12, v, attrs, out=out)
        torch.cuda.synchronize()
        assert not bool(out.any())
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
    attrs = torch.ones((300, 1), dtype=torch.float32, device=DEV)
    out = torch.zeros((1, 48, 64), dtype=torch.float32, device=DEV)
    args = (0, 3, st.act, attrs, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(), *tail)
    st.raster.optimize_rows_without_gradient(*st._state(), *st._adam_settings(), st.act, lazy=st._lazy())
    with pytest.raises(RuntimeError, match=f"{NAME}: gut_optimize_rows_without_gradient was called for this forward"):
        st.raster.trace_attributes(*args, out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())
    st.raster.finish_optimizer_step_without_gradient()                   # ends the half-applied step; then the handle goes on
    st.forward(batch)
    st.raster.trace_attributes(*args, out=out)
    torch.cuda.synchronize()
    assert bool(out.any())


def test_empty_inputs_give_zero_planes():
    case = cr.case("pinhole_64x48")
    H, W = case["H"], case["W"]
    v = _device_view(case["view"])
    raster = _raster()
    # no Gaussians
    d12, sph = torch.zeros((0, 12), device=DEV), torch.zeros((0, 48), device=DEV)
    _forward(raster, d12, sph, v)
    out = torch.full((3, H, W), 7.0, dtype=torch.float32, device=DEV)
    _render(raster, d12, v, torch.zeros((0, 3), device=DEV), out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())
    # a view that sees nothing: the scene lies behind the camera
    away = _device_view(make_view("pinhole", W, H, cams.look_at_c2w((0.3, -0.2, -4.0), (0.6, -0.4, -8.0)), fx=64.0))
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    _forward(raster, d12, sph, away)
    assert raster.stats()["num_intersections"] == 0
    out.fill_(7.0)
    _render(raster, d12, away, torch.ones((300, 3), device=DEV), out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_selection_end_to_end():
    """The CPU test's three views and truth on the device: lift_masks over two views with the reference's label masks, select,
    render_selection into the third.  The device's selection is the reference's except for rows whose reference share lies within
    (PIX_FLIP x row flip budget + COLOUR_TOL x pixels_i) / weight_sum_i of the threshold, its predicted mask the reference's except
    at pixels whose reference s(p) lies within COLOUR_TOL + PIX_FLIP x budget(p) of 0.5; each exception set is at most 5 % of the
    scored rows / the pixels (tests/test_cpu_attributes.py checks that the reference's own near sets fit)."""
    c = ar.selection_case()
    model = native.NativeGaussianModel(c["scene"], device=DEV)
    tracer = gut.Tracer({"render": {}})
    batches = [to_batch(v, DEV) for v in c["views"]]
    lifted = selection.lift_masks(model, tracer, batches[:2], [torch.as_tensor(l) for l in c["labels"][:2]])
    assert lifted["n_views"] == 2 and lifted["share"].dtype == torch.float64 and tuple(lifted["share"].shape) == (300,)
    # the order of the views does not matter: integer sums
    swapped = selection.lift_masks(model, tracer, batches[1::-1], [c["labels"][1], c["labels"][0]])
    assert torch.equal(swapped["share"], lifted["share"]) and torch.equal(swapped["pixels"], lifted["pixels"])
    selected = selection.select(lifted)
    renderer = attributes.AttributeRenderer(model, tracer)
    s = selection.render_selection(renderer, batches[2], selected)
    rgba, _ = renderer.render_with_image(batches[2], selected)
    torch.cuda.synchronize()
    assert tuple(s.shape) == (48, 64) and float(s.min()) >= 0.0 and bool((s <= rgba.reshape(48, 64, 4)[..., 3] + COLOUR_TOL).all())
    ref_share, scored = c["lifted"]["share"], c["scored"]
    near_rows = (np.abs(ref_share - 0.5) <= c["row_slack"]) & scored
    sel = selected.cpu().numpy()
    differ = sel != c["selected"]
    print(f"[selection on the device] {int(sel.sum())} selected ({int(c['selected'].sum())} by the reference), {int(differ.sum())} rows differ, "
          f"{int(near_rows.sum())} of {int(scored.sum())} scored rows near the threshold; largest share difference "
          f"{float(np.abs(lifted['share'].cpu().numpy() - ref_share)[scored].max()):.3e}")
    assert not (differ & ~near_rows).any()
    assert near_rows.sum() <= 0.05 * scored.sum()
    pred = (s > 0.5).cpu().numpy()
    near_pixels = np.abs(c["s"] - 0.5) <= c["pixel_slack"]
    assert near_pixels.sum() <= 0.05 * near_pixels.size
    assert not ((pred != c["pred"]) & ~near_pixels).any()
    iou = selection.mask_iou(pred, c["labels"][2])
    print(f"[selection on the device] IoU {iou:.6f}, the reference's {c['iou']:.6f}; {int((pred != c['pred']).sum())} pixels differ")
    assert iou > 0.5


def test_trainer_selects_by_masks(tmp_path, capsys):
    """--select-by-masks on a small synthetic COLMAP scene: 8 views of 96 x 96 (7 to train on, 1 held out), 40 iterations; the label
    files are the teacher's truth (position.x < 0) rendered on the teacher with the attribute renderer, above one half."""
    from PIL import Image
    from tests.synthetic_colmap import write_synthetic_colmap
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=8, size=96, n_teacher=20_000, n_points=2_000)
    teacher = scenes.scene_lego_like(20_000, seed=1)
    renderer = attributes.AttributeRenderer(native.NativeGaussianModel(teacher, device=DEV), gut.Tracer({"render": {}}))
    truth = torch.as_tensor(np.asarray(teacher["positions"])[:, 0] < 0)
    scene = io_colmap.ColmapScene(root, "train", 1, 0)
    for i in range(len(scene)):
        label = (renderer.render(scene.batch(i), truth)[0] > 0.5).cpu().numpy()
        assert 0 < int(label.sum()) < label.size
        stem = os.path.splitext(os.path.join(root, "images", scene.images[i].name))[0]
        Image.fromarray(label.astype(np.uint8) * 255).save(stem + "_object.png")
    del renderer
    out = str(tmp_path / "run")
    assert trainer_mod.main(["--path", root, "--n-iterations", "40", "--out-dir", out, "--select-by-masks"]) == 0
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    n, n_sel = stats["n_gaussians"], stats["selection_n_selected"]
    print(f"[trainer selection] {n_sel} of {n} rows selected from {stats['selection_n_views_lifted']} views, held-out IoU {stats['selection_mean_iou']}")
    assert stats["selection_n_views_lifted"] == 7 and stats["selection_threshold"] == 0.5 and 0 < n_sel < n
    assert 0.0 <= stats["selection_mean_iou"] <= 1.0
    sel = np.load(os.path.join(out, "selection.npy"))
    assert sel.dtype == bool and sel.shape == (n,) and int(sel.sum()) == n_sel
    assert io_ply.read_ply(os.path.join(out, "selected.ply"))["positions"].shape[0] == n_sel
    assert io_ply.read_ply(os.path.join(out, "rest.ply"))["positions"].shape[0] == n - n_sel
    renders = sorted(os.listdir(os.path.join(out, "renders_selection")))
    assert renders == ["00000.png"]
    with Image.open(os.path.join(out, "renders_selection", renders[0])) as img:
        assert img.mode == "L" and img.size == (96, 96) and np.asarray(img).max() > 0
    # without the flag: none of the keys, none of the files
    out2 = str(tmp_path / "plain")
    assert trainer_mod.main(["--path", root, "--n-iterations", "5", "--out-dir", out2]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    assert not any(k.startswith("selection") for k in plain)
    assert not os.path.exists(os.path.join(out2, "selection.npy")) and not os.path.exists(os.path.join(out2, "renders_selection"))
