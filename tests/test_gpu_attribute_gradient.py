"""gut_trace_attributes_bwd on the device: the gradient rows against the CPU reference
(tests/attribute_gradient_reference.py, asserted by tests/test_cpu_attribute_gradient.py); the properties that hold exactly, as
bits; against the clamped weighted walk; as the adjoint of gut_trace_attributes; that it disturbs nothing; its refusals; empty
inputs; autograd through AttributeRenderer; the feature fit end to end and through the trainer's command line."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import attribute_gradient_reference as gr
from tests import contribution_reference as cr
from tests import weighted_contribution_reference as wr
from tests.common import ROW_FLIP_BOUND, cams, check_gradient_rows, check_gradients_per_row, make_view, scenes, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
attributes = importlib.import_module("3dgrut_amd.attributes")
features = importlib.import_module("3dgrut_amd.features")
io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
native = importlib.import_module("3dgrut_amd.native")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
_capi = importlib.import_module("3dgrut_amd._capi")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"
PAD = 0xFFFFFFFF
NAME = "gut_trace_attributes_bwd"


def _device_view(view):
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def _raster(conf=None):
    return gut.Tracer({"render": dict(conf or {})}).tracer_wrapper


def _forward(raster, d12, sph, v):
    return raster.trace(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"])


def _render(raster, d12, v, attrs):
    return raster.trace_attributes(0, 3, d12, attrs, v["ro"], v["rd"], *v["tail"])


def _bwd(raster, d12, v, g, out=None):
    return raster.trace_attributes_bwd(0, 3, d12, g, v["ro"], v["rd"], *v["tail"], out=out)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Equal as values, and bit for bit wherever not zero (a zero sum is +0 on both sides of an identity, its negation -0)."""
    nz = a != 0
    return torch.equal(a, b) and torch.equal(_bits(a)[nz], _bits(b)[nz])


def _case_on_device(name):
    case = cr.case(name)
    raster = _raster(case["conf"])
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    return case, raster, v, d12, sph


def _unwalked_rows(raster, ref, n):
    ordered = raster.debug_buffer("ordered_ids").cpu().numpy().view(np.uint32)
    trav = raster.debug_buffer("tile_traversed_fwd").cpu().numpy().view(np.uint32)
    walked = np.zeros(n, bool)
    for t, (b0, e0) in enumerate(ref["tile_ranges"]):
        ids = ordered[b0:b0 + min(int(trav[t]), int(e0) - int(b0))]
        walked[ids[ids != PAD]] = True
    return ~walked | (ref["tiles_count"] == 0)


@pytest.mark.parametrize("name", cr.CASES)
def test_rows_against_the_reference(name):
    """The seeded cotangent in [-1, 1], K = 4: every channel of the device gradient is held to the float64 reference by the project's
    row bar (common.check_gradient_rows) with the flip budget and fp32 conditioning of the oracle backward of (g_k, 0, 0, 0)."""
    case, raster, v, d12, sph = _case_on_device(name)
    G = gr.gradient_case(name)
    n = case["d12"].shape[0]
    _forward(raster, d12, sph, v)
    grad = _bwd(raster, d12, v, _t(G["g"]))
    torch.cuda.synchronize()
    assert raster.stats()["num_intersections"] == case["ref"]["M"]
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (n, 4) and bool(torch.isfinite(grad).all())
    got = grad.cpu().numpy()
    for k in range(4):
        check_gradient_rows(got[:, k:k + 1], G["grad"][:, k:k + 1], f"attribute gradient {name} channel {k}", budget=G["flip_budget"][k],
                            noise=G["fp32_noise"][k])
    print(f"[attribute gradient {name}] largest |difference| {np.abs(got - G['grad']).max():.3e}, largest |grad| {np.abs(G['grad']).max():.3f}")
    assert float(grad.min()) < 0 < float(grad.max())


@pytest.mark.parametrize("name", ["ragged_70x45", "fisheye", "single_tile_1025"])
def test_exact_identities(name):
    """As bits: two calls; grad(-g) = -grad(g); grad(2^10 g) and grad(2^-10 g) are the exact scalings; a zero cotangent gives zeros
    and no NaN; a sentinel-filled buffer is overwritten in full; rows the forward did not walk are exactly 0; NaN and +-inf in the
    cotangent count as 0; a cotangent that does not start on a 16-byte boundary gives the bits of its aligned copy."""
    case, raster, v, d12, sph = _case_on_device(name)
    ref, n, H, W = case["ref"], case["d12"].shape[0], case["H"], case["W"]
    g = _t(np.random.default_rng(140).uniform(-1, 1, (5, H, W)))
    _forward(raster, d12, sph, v)
    a, b = _bwd(raster, d12, v, g), _bwd(raster, d12, v, g)
    assert tuple(a.shape) == (n, 5) and torch.equal(_bits(a), _bits(b)) and bool(a.any())
    assert _same_bits(_bwd(raster, d12, v, -g), -a)
    assert _same_bits(_bwd(raster, d12, v, g * 1024.0), a * 1024.0)
    assert _same_bits(_bwd(raster, d12, v, g * 2.0 ** -10), a * 2.0 ** -10)
    zero = _bwd(raster, d12, v, torch.zeros_like(g), out=torch.full((n, 5), float("nan"), device=DEV))
    assert torch.equal(_bits(zero), torch.zeros_like(_bits(zero)))
    sentinel = torch.full((n, 5), 12345.0, dtype=torch.float32, device=DEV)
    assert _bwd(raster, d12, v, g, out=sentinel) is sentinel and torch.equal(_bits(sentinel), _bits(a))
    unwalked = _unwalked_rows(raster, ref, n)
    assert (int(unwalked.sum()) > 0) == (cr.base_name(name) != "ragged_70x45")
    assert not _bits(a)[torch.as_tensor(unwalked, device=DEV)].any()
    # non-finite cotangent values count as 0: against the call with those pixels zeroed
    bad = torch.as_tensor(np.random.default_rng(141).uniform(0, 1, (5, H, W)) < 0.05, device=DEV)
    poisoned, cleaned = g.clone(), g.clone()
    poisoned[bad] = torch.as_tensor([float("nan"), float("inf"), -float("inf")], device=DEV)[torch.arange(int(bad.sum()), device=DEV) % 3]
    cleaned[bad] = 0.0
    got = _bwd(raster, d12, v, poisoned)
    assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(_bwd(raster, d12, v, cleaned)))
    assert not torch.equal(got, a)
    # a whole plane of non-finite values: zeros
    assert not _bits(_bwd(raster, d12, v, torch.full((1, H, W), float("inf"), device=DEV))).any()
    # alignment of the cotangent
    store = torch.zeros(5 * H * W + 4, dtype=torch.float32, device=DEV)
    shifted = store[1:1 + 5 * H * W].view(5, H, W)
    shifted.copy_(g)
    assert shifted.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 0 and shifted.is_contiguous()
    assert torch.equal(_bits(_bwd(raster, d12, v, shifted)), _bits(a))
    torch.cuda.synchronize()
    print(f"[attribute gradient exact {name}] {int(unwalked.sum())} of {n} rows unwalked, {int(bad.sum())} cotangent values poisoned")


def test_channel_counts():
    """K = 1, 3, 4, 5 and 9 on the ragged case: channel k of every K has the bits of a K = 1 call on that plane (one walk per group
    of four, a last group of one or three channels; every channel has its own fixed-point scale, so the planes are scaled very
    differently here and still do not see each other)."""
    case, raster, v, d12, sph = _case_on_device("ragged_70x45")
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    g = _t(np.random.default_rng(142).uniform(-1, 1, (9, H, W)))
    g *= torch.as_tensor([1.0, 1e-6, 3e4, 0.37, 1e3, 2.0 ** -20, 7.0, 1e-3, 5e5], device=DEV)[:, None, None]
    _forward(raster, d12, sph, v)
    single = [_bwd(raster, d12, v, g[k:k + 1].contiguous())[:, 0] for k in range(9)]
    for k_total in (1, 3, 4, 5, 9):
        out = _bwd(raster, d12, v, g[:k_total].contiguous())
        assert tuple(out.shape) == (n, k_total)
        for k in range(k_total):
            assert torch.equal(_bits(out[:, k]), _bits(single[k])), (k_total, k)
    torch.cuda.synchronize()
    assert all(bool(s.any()) for s in single)


@pytest.mark.parametrize("name", cr.CASES)
def test_against_the_clamped_walk(name):
    """A plane P in [0, 1], K = 1, against gut_trace_contribution_weighted's q32 sums.  Both walks form the same fp32 sum per
    (tile, chunk) flush — the same products w P, the same tree, the same wave order — and differ only in how the flush rounds it:
    to 2^-32 there (half a unit: 2^-33), to 2^-s here with s = 39 or 40 for a plane whose maximum lies in (1/2, 1] (2^-40 at most),
    and in the final conversion to fp32 here (2^-24 relative).  A row is flushed once per tile that lists it:
        |grad_i - q32_i 2^-32| <= tiles_count_i (2^-33 + 2^-40) + 2^-24 |grad_i|."""
    case, raster, v, d12, sph = _case_on_device(name)
    n = case["d12"].shape[0]
    plane = _t(wr.weighted_case(name)["plane"])
    assert 0.5 < float(plane.max()) <= 1.0 and float(plane.min()) >= 0.0
    _forward(raster, d12, sph, v)
    grad = _bwd(raster, d12, v, plane[None].contiguous())[:, 0]
    wq = torch.zeros((n,), dtype=torch.int64, device=DEV)
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], None, pixel_weight=plane, weighted=wq)
    torch.cuda.synchronize()
    diff = (grad.double() - wq.double() * 2.0 ** -32).abs().cpu().numpy()
    bound = case["ref"]["tiles_count"].astype(np.float64) * (2.0 ** -33 + 2.0 ** -40) + 2.0 ** -24 * grad.double().abs().cpu().numpy()
    print(f"[attribute gradient vs clamped walk {name}] largest difference {diff.max():.3e}, largest difference / bound "
          f"{(diff / np.maximum(bound, 1e-300)).max():.3f}, {int((wq > 0).sum())} rows scored")
    assert (diff <= bound).all() and bool(wq.any())


@pytest.mark.parametrize("name", cr.CASES)
def test_adjoint_of_the_attribute_walk(name):
    """A signed cotangent g and a signed channel a:  | sum_p g out(a) - sum_i a_i grad_i(g) | <= 2^-20 sum_p (hits(p) + 2) max|g| max|a|,
    both sides summed in float64 on the host: §15's bound, scaled (both sides sum the products w a g over the same pairs from
    bit-identical w; 2^-20 is eight half-ulps per composited term)."""
    case, raster, v, d12, sph = _case_on_device(name)
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    rng = np.random.default_rng(150 + cr.case_index(name))
    g, a = _t(rng.uniform(-3, 3, (1, H, W))), _t(rng.uniform(-2, 2, (n, 1)))
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    out = _render(raster, d12, v, a)
    grad = _bwd(raster, d12, v, g)
    torch.cuda.synchronize()
    lhs, rhs = float((g.double() * out.double()).sum()), float((a.double() * grad.double()).sum())
    bound = 2.0 ** -20 * float((hits.double() + 2.0).sum()) * float(g.abs().max()) * float(a.abs().max())
    print(f"[attribute gradient adjoint {name}] sum g out {lhs!r} vs sum a grad {rhs!r}: difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert float(grad.min()) < 0 < float(grad.max()) and float(out.min()) < 0 < float(out.max())


def test_nothing_else_changes():
    """With and without gradient calls between the forward and what follows it: the four forward outputs, the handle's gradient
    rows, the lists and depths the backward reads and the records of a following contribution call are the same, bit for bit.  The
    gradients of a following backward are compared bit for bit where that says something (two runs WITHOUT the call are the control:
    the backward compositor's float atomics arrive in no fixed order) and held to the oracle's backward by the
    project's row bar either way, as §15 does."""
    case = cr.case("pinhole_64x48")
    n, W, H = 300, case["W"], case["H"]
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    g = _t(np.random.default_rng(143).uniform(-1, 1, (6, H, W)))
    rgba_grad_host = np.random.default_rng(11).normal(size=(H, W, 4)).astype(np.float32)
    rgba_grad = torch.as_tensor(rgba_grad_host, device=DEV)
    lists = ("ordered_ids", "tile_ranges", "tile_traversed_fwd")

    def run(with_call):
        raster = _raster()
        outs = _forward(raster, d12, sph, v)
        raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.ones_like(outs[0]), outs[1], None)
        outs = _forward(raster, d12, sph, v)
        before = [o.clone() for o in outs]
        if with_call:
            _bwd(raster, d12, v, g)
            _bwd(raster, d12, v, g[:1].contiguous())
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
    same = lambda x, y: torch.equal(_bits(x[3]), _bits(y[3])) and torch.equal(_bits(x[4]), _bits(y[4]))
    worst = lambda x, y: max(float((x[3] - y[3]).abs().max()), float((x[4] - y[4]).abs().max()))
    print(f"[attribute gradient disturbs nothing] gradients of two runs without the call bit-identical: {same(plain, control)} (largest "
          f"difference {worst(plain, control):.3e}); with and without the call: {same(plain, touched)} (largest difference {worst(plain, touched):.3e})")
    if same(plain, control):
        assert same(plain, touched)
    dens_g, sph_g, _, budget = oracle.backward(case["view"]["oracle_cam"], case["ref"], rgba_grad_host, np.zeros((H, W, 1), np.float32),
                                               flip_bound=ROW_FLIP_BOUND)
    check_gradients_per_row(touched[3].cpu().numpy(), touched[4].cpu().numpy(), dens_g, sph_g, "backward after trace_attributes_bwd", budget=budget)


def _raw_call(raster, n, d12, v, k, g_ptr, grad_ptr, stream=None):
    cam = raster._camera(*v["tail"])
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    H, W = int(v["ro"].shape[1]), int(v["ro"].shape[2])
    return raster._lib.gut_trace_attributes_bwd(raster._handle, C.c_void_p(st), 0, 3, n, d12.data_ptr(), W, H, v["ro"].data_ptr(),
                                                v["rd"].data_ptr(), C.byref(cam), k, g_ptr, grad_ptr)


def test_refusals_leave_the_handle_rendering():
    case, other = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n, H, W = 300, case["H"], case["W"]
    v, vo = _device_view(case["view"]), _device_view(other["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    g = _t(np.random.default_rng(144).uniform(-1, 1, (2, H, W)))
    raster = _raster()
    out = torch.zeros((n, 2), dtype=torch.float32, device=DEV)

    fresh = _raster()
    _forward(fresh, d12, sph, v)
    want = _bwd(fresh, d12, v, g)
    state = dict(forwarded=False)

    def refused(pattern, call, error=RuntimeError):
        with pytest.raises(error, match=pattern):
            call()
        torch.cuda.synchronize()
        assert not bool(out.any()), f"{pattern!r}: the refused call wrote"
        if state["forwarded"]:       # after each refusal the handle still differentiates the case as an untouched one does
            assert torch.equal(_bits(_bwd(raster, d12, v, g)), _bits(want)), pattern

    def raw(*a, **kw):
        _capi.check(_raw_call(raster, *a, **kw), "trace_attributes_bwd")

    refused(re.escape(f"{NAME}: no forward context on this stream"), lambda: _bwd(raster, d12, v, g, out=out))
    ref_out = [o.clone() for o in _forward(raster, d12, sph, v)]
    state["forwarded"] = True
    side = torch.cuda.Stream(DEV)
    refused(re.escape(f"{NAME}: no forward context on this stream"),
            lambda: raw(n, d12, v, 2, g.data_ptr(), out.data_ptr(), stream=side.cuda_stream))
    refused(re.escape(f"{NAME}: camera differs from the cached forward"),
            lambda: raster.trace_attributes_bwd(0, 3, d12, g, v["ro"], v["rd"], *vo["tail"], out=out))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 0"), lambda: raw(n, d12, v, 0, g.data_ptr(), out.data_ptr()))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 65"), lambda: raw(n, d12, v, 65, g.data_ptr(), out.data_ptr()))
    refused(re.escape(f"{NAME}: d_out_grad is NULL"), lambda: raw(n, d12, v, 2, None, out.data_ptr()))
    refused(re.escape(f"{NAME}: d_attributes_grad is NULL"), lambda: raw(n, d12, v, 2, g.data_ptr(), None))
    refused(re.escape(f"{NAME}: d_out_grad must be 4-byte aligned"), lambda: raw(n, d12, v, 2, g.data_ptr() + 2, out.data_ptr()))
    refused(re.escape(f"{NAME}: d_attributes_grad must be 4-byte aligned"), lambda: raw(n, d12, v, 2, g.data_ptr(), out.data_ptr() + 2))
    refused(re.escape(f"{NAME}: arguments differ from the cached forward"), lambda: raw(n - 1, d12, v, 2, g.data_ptr(), out.data_ptr()))
    # the Python surface checks its tensors before the library sees them
    for bad in (g[:, :H - 1], g[0], g.double(), g.cpu(), g.permute(0, 2, 1).contiguous().permute(0, 2, 1), g.to(torch.int32)):
        refused(r"attribute cotangent: a contiguous float32 tensor \[K, 48, 64\]", lambda: _bwd(raster, d12, v, bad, out=out))
    for bad_out in (torch.zeros((n, 3), device=DEV), torch.zeros((n, 2), dtype=torch.float64, device=DEV), torch.zeros((2, n), device=DEV)):
        refused("attribute gradient", lambda: _bwd(raster, d12, v, g, out=bad_out))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 0"), lambda: _bwd(raster, d12, v, g[:0].contiguous()))
    refused(re.escape(f"{NAME}: num_channels must be in 1..64, got 65"), lambda: _bwd(raster, d12, v, torch.zeros((65, H, W), device=DEV)))
    # the handle still renders, and differentiates, as an untouched one
    got = _bwd(raster, d12, v, g)
    again = _forward(raster, d12, sph, v)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)) and bool(got.any())
    for o, b in zip(again, ref_out):
        assert torch.equal(o, b)

    for conf, what in (({"splat": {"k_buffer_size": 16}}, "k_buffer_size=16"), ({"particle_kernel_degree": 4}, "particle_kernel_degree=4")):
        r = _raster(conf)
        outs = [o.clone() for o in _forward(r, d12, sph, v)]
        with pytest.raises(RuntimeError, match=re.escape(f"{NAME}: supported on the unsorted variant (k_buffer_size=0) at particle_kernel_degree=2 only") + ".*" + re.escape(what)):
            _bwd(r, d12, v, g, out=out)
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
    g = torch.ones((1, 48, 64), dtype=torch.float32, device=DEV)
    out = torch.zeros((300, 1), dtype=torch.float32, device=DEV)
    args = (0, 3, st.act, g, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(), *tail)
    st.raster.optimize_rows_without_gradient(*st._state(), *st._adam_settings(), st.act, lazy=st._lazy())
    with pytest.raises(RuntimeError, match=f"{NAME}: gut_optimize_rows_without_gradient was called for this forward"):
        st.raster.trace_attributes_bwd(*args, out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())
    st.raster.finish_optimizer_step_without_gradient()                   # ends the half-applied step; then the handle goes on
    st.forward(batch)
    st.raster.trace_attributes_bwd(*args, out=out)
    torch.cuda.synchronize()
    assert bool(out.any())


def test_empty_inputs_give_zero_rows():
    case = cr.case("pinhole_64x48")
    H, W = case["H"], case["W"]
    v = _device_view(case["view"])
    raster = _raster()
    g = torch.ones((3, H, W), dtype=torch.float32, device=DEV)
    # no Gaussians
    d12, sph = torch.zeros((0, 12), device=DEV), torch.zeros((0, 48), device=DEV)
    _forward(raster, d12, sph, v)
    assert tuple(_bwd(raster, d12, v, g).shape) == (0, 3)
    # a view that sees nothing: the scene lies behind the camera
    away = _device_view(make_view("pinhole", W, H, cams.look_at_c2w((0.3, -0.2, -4.0), (0.6, -0.4, -8.0)), fx=64.0))
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    _forward(raster, d12, sph, away)
    assert raster.stats()["num_intersections"] == 0
    out = torch.full((300, 3), 7.0, dtype=torch.float32, device=DEV)
    _bwd(raster, d12, away, g, out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_autograd_through_the_renderer():
    """render(batch, a.requires_grad_()).backward(g): a.grad has the bits of the raw call and the planes those of the
    non-differentiable render; a backward taken after another view was rendered on the same renderer runs its own forward again and
    gives the same bits; attributes without grad build no graph; a 1-D attribute tensor gets a 1-D gradient."""
    case, other = cr.case("ragged_70x45"), cr.case("pinhole_64x48")
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    model = native.NativeGaussianModel(scenes.scene_c1(333, 0), device=DEV)
    renderer = attributes.AttributeRenderer(model, gut.Tracer({"render": {}}))
    batch = to_batch(case["view"], DEV)
    other_batch = to_batch(make_view("pinhole", 64, 48, cams.orbit_c2w(4.0, -25.0, 5.0), fx=64.0), DEV)
    rng = np.random.default_rng(145)
    a0, g = _t(rng.uniform(-1, 1, (n, 5))), _t(rng.uniform(-1, 1, (5, H, W)))
    plain = renderer.render(batch, a0)
    assert not plain.requires_grad and plain.grad_fn is None
    # the raw call on the renderer's own forward
    _, rays_o, rays_d, cam = renderer.forward(batch)
    raw = renderer.raster.trace_attributes_bwd(0, renderer.n_active_features, renderer.act, g, rays_o, rays_d, *cam)
    a = a0.clone().requires_grad_(True)
    rgba, planes = renderer.render_with_image(batch, a)
    assert planes.requires_grad and not rgba.requires_grad and torch.equal(_bits(planes.detach()), _bits(plain))
    planes.backward(g)
    assert torch.equal(_bits(a.grad), _bits(raw)) and bool(a.grad.any())
    # another view in between: the backward forwards its own batch again
    b = a0.clone().requires_grad_(True)
    planes = renderer.render(batch, b)
    count = renderer.n_forwards
    renderer.render(other_batch, a0)
    planes.backward(g)
    assert renderer.n_forwards == count + 2 and torch.equal(_bits(b.grad), _bits(raw))
    # through further torch operations, and a 1-D tensor
    c = a0[:, 0].clone().requires_grad_(True)
    (renderer.render(batch, 2.0 * c) * g[:1]).sum().backward()
    assert tuple(c.grad.shape) == (n,) and torch.equal(c.grad, 2.0 * raw[:, 0])
    with torch.no_grad():
        assert not renderer.render(batch, a).requires_grad
    assert all(p.grad is None for p in (model.raw, model.features) if isinstance(p, torch.Tensor))
    torch.cuda.synchronize()


def test_fit_reaches_the_held_out_view():
    """The reference fit's scene and settings (tests/attribute_gradient_reference.fit_case: 300 Gaussians, three 64 x 48 views, two
    fitted, Adam at 0.03 from zero, 200 iterations) on the device through features.fit_features with the default loss on the
    un-premultiplied target maps: the held-out view's MSE against W a* is at most 1e-2 of the zero fit's.  The distance to the float64
    reference fit is printed, not asserted (200 fp32 Adam steps have no derived bar); MEASURED on one MI355X: see DESIGN.md §17."""
    f = gr.fit_case()
    model = native.NativeGaussianModel(f["scene"], device=DEV)
    renderer = attributes.AttributeRenderer(model, gut.Tracer({"render": {}}))
    batches = [to_batch(v, DEV) for v in f["views"]]
    maps = [_t(m) for m in f["maps"]]
    fitted = features.fit_features(renderer, batches[:2], maps[:2], 4, gr.FIT_ITERATIONS, gr.FIT_LR)
    assert fitted.dtype == torch.float32 and tuple(fitted.shape) == (300, 4) and not fitted.requires_grad
    held = renderer.render(batches[2], fitted)
    zero = renderer.render(batches[2], torch.zeros_like(fitted))
    want = torch.as_tensor(f["rendered"][2], device=DEV)
    mse, zero_mse = float(((held.double() - want) ** 2).mean()), float(((zero.double() - want) ** 2).mean())
    scored = features.score_features(renderer, batches[2:], maps[2:], fitted)
    ref_planes = (f["matrices"][2] @ f["fitted"]).T.reshape(4, 48, 64)
    print(f"[feature fit on the device] held-out MSE {mse:.3e} against the zero fit's {zero_mse:.3e}: {mse / zero_mse:.3e} x (the float64 "
          f"reference: {f['heldout_mse'] / f['zero_mse']:.3e} x); score_features {float(scored[0]):.3e}; distance to the reference fit: rows "
          f"{float(np.abs(fitted.cpu().numpy() - f['fitted']).max()):.3e}, held-out planes {float(np.abs(held.cpu().numpy() - ref_planes).max()):.3e}")
    assert mse <= 1e-2 * zero_mse
    assert tuple(scored.shape) == (1,) and scored.dtype == torch.float64 and float(scored[0]) <= 1e-2 * zero_mse
    # a callable loss and a start other than zero: one step from the fitted rows on the plain squared error moves them
    moved = features.fit_features(renderer, batches[:1], [want.float()], 4, 1, 1e-3, init=fitted,
                                  loss=lambda out, alpha, target: ((out - target) ** 2).sum())
    assert float((moved - fitted).abs().max()) > 0 and float((moved - fitted).abs().max()) <= 1.001e-3


def test_trainer_fits_features(tmp_path, capsys):
    """--fit-features on a small synthetic COLMAP scene: 8 views of 96 x 96 (7 to train on, 1 held out), 40 iterations; the map
    files are planted features of the teacher, (sin 2x, [x < 0]), rendered on the teacher with the attribute renderer and divided by
    its alpha.  The trained model is another one, so the fit cannot be exact: the held-out score must beat the zero fit's."""
    from tests.synthetic_colmap import write_synthetic_colmap
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=8, size=96, n_teacher=20_000, n_points=2_000)
    teacher = scenes.scene_lego_like(20_000, seed=1)
    renderer = attributes.AttributeRenderer(native.NativeGaussianModel(teacher, device=DEV), gut.Tracer({"render": {}}))
    pos = np.asarray(teacher["positions"], np.float64)
    planted = _t(np.stack([np.sin(2.0 * pos[:, 0]), (pos[:, 0] < 0).astype(np.float64)], axis=1))
    zero_mse = None
    for split in ("train", "test"):
        scene = io_colmap.ColmapScene(root, split, 1, 8)
        for i in range(len(scene)):
            rgba, planes = renderer.render_with_image(scene.batch(i), planted)
            alpha = rgba.reshape(96, 96, 4)[..., 3]
            fmap = torch.where(alpha[None] > 1e-3, planes / alpha[None].clamp_min(1e-3), torch.zeros_like(planes))
            stem = os.path.splitext(os.path.join(root, "images", scene.images[i].name))[0]
            np.save(stem + "_planted.npy", fmap.cpu().numpy())
            if split == "test":
                held_stem, held_map = os.path.basename(stem), fmap
    del renderer
    out = str(tmp_path / "run")

    captured = {}
    real_init = trainer_mod.Trainer.fit_features

    def spy(self):
        captured["before"] = [t.detach().clone() for t in (self.model.raw, self.model.features)]
        res = real_init(self)
        captured["after"] = [t.detach().clone() for t in (self.model.raw, self.model.features)]
        from importlib import import_module
        r = import_module("3dgrut_amd.attributes").AttributeRenderer(self.model, self.tracer)
        b = self.test_batches[0]
        captured["zero"] = float(features.score_features(r, [b], [b.feature_map], torch.zeros((int(self.model.num_gaussians), 2), device=DEV))[0])
        return res
    trainer_mod.Trainer.fit_features = spy
    try:
        assert trainer_mod.main(["--path", root, "--n-iterations", "40", "--out-dir", out, "--fit-features", "_planted",
                                 "--feature-iterations", "60", "--feature-lr", "0.05"]) == 0
    finally:
        trainer_mod.Trainer.fit_features = real_init
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    with capsys.disabled():
        print(f"[trainer features] {stats['features_channels']} channels fitted on {stats['features_n_views_fitted']} views: train MSE "
              f"{stats['features_train_mse']:.3e}, held-out MSE {stats['features_heldout_mse']:.3e} against the zero fit's {captured['zero']:.3e}")
    assert stats["features_channels"] == 2 and stats["features_n_views_fitted"] == 7
    assert 0.0 <= stats["features_train_mse"] and stats["features_heldout_mse"] < captured["zero"]
    for x, y in zip(captured["before"], captured["after"]):
        assert torch.equal(_bits(x), _bits(y))
    n = stats["n_gaussians"]
    fitted = np.load(os.path.join(out, "features.npy"))
    assert fitted.dtype == np.float32 and fitted.shape == (n, 2) and np.isfinite(fitted).all() and np.abs(fitted).max() > 0
    assert sorted(os.listdir(os.path.join(out, "renders_features"))) == [held_stem + ".npy"]
    planes = np.load(os.path.join(out, "renders_features", held_stem + ".npy"))
    assert planes.dtype == np.float32 and planes.shape == (2, 96, 96) and np.abs(planes).max() > 0
    # a map of another size is refused; without the flag: none of the keys, none of the files
    bad_root = str(tmp_path / "run_bad")
    stem0 = os.path.splitext(os.path.join(root, "images", io_colmap.ColmapScene(root, "train", 1, 8).images[0].name))[0]
    good = np.load(stem0 + "_planted.npy")
    np.save(stem0 + "_planted.npy", good[:, :-1])
    with pytest.raises(ValueError, match="feature map"):
        trainer_mod.main(["--path", root, "--n-iterations", "2", "--out-dir", bad_root, "--fit-features", "_planted"])
    np.save(stem0 + "_planted.npy", good)
    out2 = str(tmp_path / "plain")
    assert trainer_mod.main(["--path", root, "--n-iterations", "5", "--out-dir", out2]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    assert not any(k.startswith("features") for k in plain)
    assert not os.path.exists(os.path.join(out2, "features.npy")) and not os.path.exists(os.path.join(out2, "renders_features"))
