"""gut_trace_contribution_weighted and gut_pixel_error on the device: the per-Gaussian sum of blending weight x a
per-pixel plane against the CPU oracle (tests/weighted_contribution_reference.py, asserted by tests/test_cpu_weighted_contribution.py)
and against the device's own forward; the identities that hold exactly, as integers; bit reproducibility; that it disturbs nothing;
its refusals; the error plane against its float64 definition; ContributionScores.accumulate_error end to end."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import weighted_contribution_reference as wr
from tests.common import COLOUR_TOL, ROW_FLIP_BOUND, cams, check_gradient_rows, check_gradients_per_row, make_view, scenes, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
contribution = importlib.import_module("3dgrut_amd.contribution")
losses = importlib.import_module("3dgrut_amd.losses")
native = importlib.import_module("3dgrut_amd.native")
strategy = importlib.import_module("3dgrut_amd.strategy")
_capi = importlib.import_module("3dgrut_amd._capi")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"
PAD = 0xFFFFFFFF
SENTINEL = 0x0123456789ABCDEF


def _device_view(view):
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]))


def _raster(conf=None):
    return gut.Tracer({"render": dict(conf or {})}).tracer_wrapper


def _records(n):
    return torch.zeros((n, 2), dtype=torch.int64, device=DEV)


def _q32(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int64, device=DEV)


def _forward(raster, d12, sph, v):
    return raster.trace(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"])


def _plain(raster, d12, v, scores):
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores)
    return scores


def _weighted(raster, d12, v, plane, weighted, scores=None):
    """The <records, weighted> walk with `scores`, the weighted-only walk without."""
    raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *v["tail"], scores, pixel_weight=plane, weighted=weighted)
    return weighted


def _plane(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _case_on_device(name):
    case = cr.case(name)
    raster = _raster(case["conf"])
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    return case, raster, v, d12, sph


@pytest.mark.parametrize("name", cr.CASES)
def test_weighted_scores_of_one_view(name):
    """The seeded uniform plane.  weighted_sum is held to the bar of weight_sum (0 <= e <= 1: every term is at most the plain one):
    common.check_gradient_rows against the oracle backward's d(sum of P * red)/d(red feature) with that call's flip budget; the total
    against the device's own sum of P * alpha; the records of the same walk equal a plain call's; unwalked rows keep their bytes."""
    case, raster, v, d12, sph = _case_on_device(name)
    w = wr.weighted_case(name)
    ref, n = case["ref"], case["d12"].shape[0]
    plane = _plane(w["plane"])
    rgba, dist, hits, vis = _forward(raster, d12, sph, v)
    scores = _records(n)
    wq = _weighted(raster, d12, v, plane, _q32(n), scores)
    plain = _plain(raster, d12, v, _records(n))
    over = _weighted(raster, d12, v, plane, _q32(n, SENTINEL), _records(n))
    torch.cuda.synchronize()
    assert raster.stats()["num_intersections"] == ref["M"]
    assert torch.equal(scores, plain) and bool(plain.any())
    assert bool((wq >= 0).all()) and bool((wq <= scores[:, 0]).all())
    ws = wq.cpu().numpy().astype(np.float64) * 2.0 ** -32

    check_gradient_rows(ws[:, None], w["feat_grad"][:, None], f"weighted contribution {name}", budget=w["flip_budget"], noise=w["fp32_noise"])

    p_alpha = float((plane.double() * rgba[..., 3].double()).sum())
    with_hit = int((hits > 0).sum())
    print(f"[weighted contribution {name}] sum of weighted_sum {ws.sum():.6f} vs sum of P * alpha {p_alpha:.6f} "
          f"(bound {COLOUR_TOL * with_hit:.3e}, {with_hit} pixels with a hit)")
    assert abs(ws.sum() - p_alpha) <= COLOUR_TOL * with_hit

    # accumulated into: integer adds on whatever was there; rows the forward did not walk keep their bytes
    assert torch.equal(over - SENTINEL, wq)
    ordered = raster.debug_buffer("ordered_ids").cpu().numpy().view(np.uint32)
    trav = raster.debug_buffer("tile_traversed_fwd").cpu().numpy().view(np.uint32)
    walked = np.zeros(n, bool)
    for t, (b, e) in enumerate(ref["tile_ranges"]):
        ids = ordered[b:b + min(int(trav[t]), int(e) - int(b))]
        walked[ids[ids != PAD]] = True
    unwalked = ~walked | (ref["tiles_count"] == 0)
    assert (over.cpu().numpy()[unwalked] == SENTINEL).all() and not wq.cpu().numpy()[unwalked].any()
    print(f"[weighted contribution {name}] {int(unwalked.sum())} of {n} rows unwalked and untouched, {int((wq > 0).sum())} scored")


@pytest.mark.parametrize("name", ["ragged_70x45", "single_tile_1025"])
def test_exact_identities(name):
    case, raster, v, d12, sph = _case_on_device(name)
    n, H, W = case["d12"].shape[0], case["H"], case["W"]
    _forward(raster, d12, sph, v)
    scores = _plain(raster, d12, v, _records(n))
    const = lambda x: torch.full((H, W), x, dtype=torch.float32, device=DEV)
    # a plane of ones is the plain sum, bit for bit; values above 1 count as 1
    ones = _weighted(raster, d12, v, const(1.0), _q32(n))
    assert torch.equal(ones, scores[:, 0]) and bool(ones.any())
    assert torch.equal(_weighted(raster, d12, v, const(2.0), _q32(n)), ones)
    assert torch.equal(_weighted(raster, d12, v, const(float("inf")), _q32(n)), ones)
    # zero, NaN and negative planes add nothing to what is there
    for x in (0.0, float("nan"), -1.0):
        assert bool((_weighted(raster, d12, v, const(x), _q32(n, SENTINEL)) == SENTINEL).all()), x
    # a tile-constant indicator and its complement split the plain sum exactly, as integers
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    P = ((tx + ty) % 2 == 0).astype(np.float32)
    a, b = _weighted(raster, d12, v, _plane(P), _q32(n)), _weighted(raster, d12, v, _plane(1.0 - P), _q32(n))
    assert torch.equal(a + b, scores[:, 0])
    if case["ref"]["tile_ranges"].shape[0] > 1:      # (a single tile lies whole in one of the two planes)
        assert bool(a.any()) and bool(b.any())
    # the weighted-only walk gives the array of the walk that writes both
    plane = _plane(wr.weighted_case(name)["plane"])
    both = _weighted(raster, d12, v, plane, _q32(n), _records(n))
    only = _weighted(raster, d12, v, plane, _q32(n))
    torch.cuda.synchronize()
    assert torch.equal(only, both) and bool(both.any()) and not torch.equal(both, ones)


def test_identical_inputs_give_identical_bits():
    a, b = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n = 300
    raster = _raster()
    d12, sph = torch.as_tensor(a["d12"], device=DEV), torch.as_tensor(a["sph"], device=DEV)   # one model, the two cases' views
    va, vb = _device_view(a["view"]), _device_view(b["view"])
    pa, pb = _plane(wr.weighted_case("pinhole_64x48")["plane"]), _plane(wr.weighted_case("ragged_70x45")["plane"])

    _forward(raster, d12, sph, va)
    s1, s2 = _weighted(raster, d12, va, pa, _q32(n)), _weighted(raster, d12, va, pa, _q32(n))     # two calls after one forward
    assert torch.equal(s1, s2) and bool(s1.any())
    _forward(raster, d12, sph, vb)
    sb = _weighted(raster, d12, vb, pb, _q32(n))
    ab = _weighted(raster, d12, vb, pb, s1.clone())                                              # A then B
    _forward(raster, d12, sph, va)
    ba = _weighted(raster, d12, va, pa, sb.clone())                                              # B then A
    torch.cuda.synchronize()
    assert torch.equal(ab, ba) and torch.equal(ab, s1 + sb)


def test_nothing_else_changes():
    case = cr.case("pinhole_64x48")
    n, W, H = 300, case["W"], case["H"]
    raster = _raster()
    v = _device_view(case["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    plane = _plane(wr.weighted_case("pinhole_64x48")["plane"])
    # (a first forward and backward, so that the handle has gradient rows to show: every consumer leaves them zero)
    outs = _forward(raster, d12, sph, v)
    raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.ones_like(outs[0]), outs[1], None)
    outs = _forward(raster, d12, sph, v)
    before = [o.clone() for o in outs]
    plane_before = plane.clone()
    _weighted(raster, d12, v, plane, _q32(n), _records(n))
    _weighted(raster, d12, v, plane, _q32(n))
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b)
    assert torch.equal(plane, plane_before)
    assert not bool(raster.debug_buffer("grad_scratch").any())
    # a backward follows as if nothing had happened
    rgba_grad = np.random.default_rng(11).normal(size=(H, W, 4)).astype(np.float32)
    g12, g48 = raster.trace_bwd(0, 3, d12, sph, v["ro"], v["rd"], None, *v["tail"], outs[0], torch.as_tensor(rgba_grad, device=DEV), outs[1], None)
    dens_g, sph_g, _, budget = oracle.backward(case["view"]["oracle_cam"], case["ref"], rgba_grad, np.zeros((H, W, 1), np.float32),
                                               flip_bound=ROW_FLIP_BOUND)
    check_gradients_per_row(g12.cpu().numpy(), g48.cpu().numpy(), dens_g, sph_g, "backward after trace_contribution_weighted", budget=budget)


def _raw_call(raster, n, d12, v, plane_ptr, scores_ptr, weighted_ptr, stream=None):
    cam = raster._camera(*v["tail"])
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    H, W = int(v["ro"].shape[1]), int(v["ro"].shape[2])
    return raster._lib.gut_trace_contribution_weighted(raster._handle, C.c_void_p(st), 0, 3, n, d12.data_ptr(), W, H, v["ro"].data_ptr(),
                                                       v["rd"].data_ptr(), C.byref(cam), plane_ptr, scores_ptr, weighted_ptr)


def test_refusals_leave_the_handle_rendering():
    case, other = cr.case("pinhole_64x48"), cr.case("ragged_70x45")
    n, H, W = 300, case["H"], case["W"]
    v, vo = _device_view(case["view"]), _device_view(other["view"])
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    plane = _plane(wr.weighted_case("pinhole_64x48")["plane"])
    raster = _raster()
    sentinel, records = _q32(n + 1), _records(n)       # (one element more: the misaligned call's array stays inside it)
    name = "gut_trace_contribution_weighted"

    def refused(pattern, call):
        with pytest.raises(RuntimeError, match=pattern):
            call()
        torch.cuda.synchronize()
        assert not bool(sentinel.any()) and not bool(records.any()), f"{pattern!r}: the refused call wrote"

    def raw(*a, **kw):
        _capi.check(_raw_call(raster, *a, **kw), "trace_contribution_weighted")

    refused(re.escape(f"{name}: no forward context on this stream"), lambda: _weighted(raster, d12, v, plane, sentinel[:n], records))
    ref_out = [o.clone() for o in _forward(raster, d12, sph, v)]
    side = torch.cuda.Stream(DEV)
    refused(re.escape(f"{name}: no forward context on this stream"),
            lambda: raw(n, d12, v, plane.data_ptr(), records.data_ptr(), sentinel.data_ptr(), stream=side.cuda_stream))
    refused(re.escape(f"{name}: camera differs from the cached forward"),
            lambda: raster.trace_contribution(0, 3, d12, v["ro"], v["rd"], *vo["tail"], records, pixel_weight=plane, weighted=sentinel[:n]))
    refused(re.escape(f"{name}: d_pixel_weight is NULL"), lambda: raw(n, d12, v, None, records.data_ptr(), sentinel.data_ptr()))
    refused(re.escape(f"{name}: d_weighted_q32 is NULL"), lambda: raw(n, d12, v, plane.data_ptr(), records.data_ptr(), None))
    refused(re.escape(f"{name}: d_weighted_q32 must be 8-byte aligned"),
            lambda: raw(n, d12, v, plane.data_ptr(), records.data_ptr(), sentinel.data_ptr() + 4))
    refused(re.escape(f"{name}: d_scores must be 8-byte aligned"),
            lambda: raw(n, d12, v, plane.data_ptr(), records.data_ptr() + 4, sentinel.data_ptr()))
    # the Python surface checks its tensors before the library sees them
    with pytest.raises(RuntimeError, match="pixel weight"):
        _weighted(raster, d12, v, plane[:, :W - 1], sentinel[:n])
    with pytest.raises(RuntimeError, match="weighted contribution"):
        _weighted(raster, d12, v, plane, sentinel)
    # the handle still scores and renders as an untouched one
    got = _weighted(raster, d12, v, plane, _q32(n))
    fresh = _raster()
    _forward(fresh, d12, sph, v)
    want = _weighted(fresh, d12, v, plane, _q32(n))
    again = _forward(raster, d12, sph, v)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(got.any())
    for o, b in zip(again, ref_out):
        assert torch.equal(o, b)

    for conf, what in (({"splat": {"k_buffer_size": 16}}, "k_buffer_size=16"), ({"particle_kernel_degree": 4}, "particle_kernel_degree=4")):
        r = _raster(conf)
        out = [o.clone() for o in _forward(r, d12, sph, v)]
        with pytest.raises(RuntimeError, match=re.escape("supported on the unsorted variant (k_buffer_size=0) at particle_kernel_degree=2 only") + ".*" + re.escape(what)):
            _weighted(r, d12, v, plane, sentinel[:n], records)
        torch.cuda.synchronize()
        assert not bool(sentinel.any()) and not bool(records.any())
        for o, b in zip(_forward(r, d12, sph, v), out):
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
    plane = torch.full((48, 64), 0.5, dtype=torch.float32, device=DEV)
    sentinel = _q32(300)
    args = (0, 3, st.act, batch.rays_ori.contiguous(), batch.rays_dir.contiguous(), *tail, None)
    st.raster.optimize_rows_without_gradient(*st._state(), *st._adam_settings(), st.act, lazy=st._lazy())
    with pytest.raises(RuntimeError, match="gut_trace_contribution_weighted: gut_optimize_rows_without_gradient was called for this forward"):
        st.raster.trace_contribution(*args, pixel_weight=plane, weighted=sentinel)
    torch.cuda.synchronize()
    assert not bool(sentinel.any())
    st.raster.finish_optimizer_step_without_gradient()                   # ends the half-applied step; then the handle goes on
    st.forward(batch)
    st.raster.trace_contribution(*args, pixel_weight=plane, weighted=sentinel)
    torch.cuda.synchronize()
    assert bool(sentinel.any())


def _error_tolerance(background_is_zero, with_exposure, with_mask):
    """(roundings, largest intermediate magnitude) of the kernel's expression for one form, inputs in [0, 1] and |E| <= 2."""
    comp_max = 1.0 if background_is_zero else 2.0
    roundings = (0 if background_is_zero else 7) + (9 if with_exposure else 0) + 3 + 2 + 1 + (1 if with_mask else 0)
    img_max = 6.0 * comp_max + 2.0 if with_exposure else comp_max
    return roundings, 3.0 * (img_max + 1.0)


def test_pixel_error_against_its_definition():
    """gut_pixel_error at 37 x 29 (no multiple of the workgroup's 256 pixels: 1073 = 4 * 256 + 49) against losses.pixel_error, the
    float64 definition on the same float32 inputs, for a constant background of 0 and of 1 and a background plane, each with and
    without a mask and an exposure.  Inputs are in [0, 1], |E| <= 2.

    The tolerance of a form is (fp32 roundings of the kernel's expression) x 2^-24 x (largest intermediate magnitude M):
      roundings  1 - alpha and, per channel, B * (1 - alpha) and its sum with rgb: 7 — none over a background of 0, where comp = rgb;
                 with E three fused multiply-adds per channel: 9; the three differences: 3; their sum: 2; the division by 3
                 (correctly rounded): 1; the mask factor: 1.  (Where the compiler fuses a product into a sum there are fewer.)
      M          comp <= 2 (1 over a background of 0); |img| <= 6 comp + 2 with E (three |A| <= 2 and |b| <= 2), comp without;
                 a difference <= |img| + 1, their sum <= 3 (|img| + 1) = M: 6 or 9 without E, 27 or 45 with it.
    A rounding moves its own result by at most 2^-24 of that result's magnitude <= 2^-24 M, and reaches the error through factors of
    at most 1 except the roundings of comp and 1 - alpha, which E amplifies by at most 6 — on values <= 2 <= M / 6.  The clamp is
    1-Lipschitz.  So |kernel - definition| <= roundings x 2^-24 x M; nothing here was tuned to what the kernel gives.
    Masked pixels are exactly 0, and a render equal to its photo (background 0, no E) gives exactly 0."""
    H, W = 37, 29
    rng = np.random.default_rng(23)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    rgba, gt = t(rng.uniform(0, 1, (H, W, 4))), t(rng.uniform(0, 1, (H, W, 3)))
    bg_plane = t(rng.uniform(0, 1, (H, W, 3)))
    mask = t(rng.choice([0.0, 0.5, 1.0], size=(H, W), p=[0.3, 0.2, 0.5]))
    E = t(rng.uniform(-2, 2, (3, 4)))
    assert int((mask == 0).sum()) > 100
    for bg_name, bg in (("0", 0.0), ("1", 1.0), ("plane", bg_plane)):
        for m in (None, mask):
            for e in (None, E):
                got = losses.fused_pixel_error(rgba, gt, bg, mask=m, exposure=e)
                want = losses.pixel_error(rgba, gt, bg, mask=m, exposure=e)
                roundings, M = _error_tolerance(bg_name == "0", e is not None, m is not None)
                tol = roundings * 2.0 ** -24 * M
                worst = float((got.double() - want).abs().max())
                print(f"[pixel error] background {bg_name}, mask {m is not None}, exposure {e is not None}: worst {worst:.3e}, "
                      f"tolerance {tol:.3e} ({roundings} roundings x 2^-24 x {M:g}); mean {float(want.mean()):.4f}, "
                      f"clamped {int((want >= 1.0).sum())}")
                assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
                assert worst <= tol
                assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float(want.mean()) > 0.05
                if m is not None:
                    assert not bool(got[m == 0].any()) and bool(got[m != 0].any())
    same = losses.fused_pixel_error(rgba, rgba[..., :3].contiguous(), 0.0)
    out = torch.full((H, W), 7.0, dtype=torch.float32, device=DEV)
    assert losses.fused_pixel_error(rgba, rgba[..., :3].contiguous(), "black", out=out) is out
    torch.cuda.synchronize()
    assert not bool(same.any()) and not bool(out.any())


def test_accumulate_error_on_a_model_that_is_its_own_photo():
    """300 rows, two views at 64 x 48.  The photos are the device's own renders of the packed rows the scorer holds, so the error
    plane is exactly 0: every weighted_sum is 0 and select_by_error selects nothing.  Then the degree-0 SH coefficients of a seeded
    10 % of the rows are raised by 0.5: among the rows that are drawn at all, the changed ones have the larger median error_mean —
    the control, the same statistic over the unchanged rows, is computed here from the same pass."""
    sc = scenes.scene_c1(300, 0)
    model = native.NativeGaussianModel(sc, device=DEV)
    tracer = gut.Tracer({"render": {}})
    views = [make_view("pinhole", 64, 48, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)), fx=64.0),
             make_view("pinhole", 64, 48, cams.orbit_c2w(4.0, 37.0, 12.0), fx=64.0)]
    batches = [to_batch(v, DEV) for v in views]
    scorer = contribution.ContributionScores(model, tracer)
    for b in batches:
        sensor, poses = scorer._create_camera(b)
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        rgba = scorer.raster.trace(0, scorer.n_active_features, scorer.act, scorer.features, b.rays_ori.contiguous(), b.rays_dir.contiguous(),
                                   None, *cam)[0]
        b.rgb_gt = rgba[..., :3].clone().contiguous()[None]
    for b in batches:
        scorer.accumulate_error(b, "black")
    res = scorer.result()
    assert res["n_views"] == 2 and res["weighted_sum"].dtype == torch.float64 and tuple(res["weighted_sum"].shape) == (300,)
    assert int((res["pixels"] > 0).sum()) > 100
    assert not bool(res["weighted_sum"].any())
    assert not bool(strategy.select_by_error(res, 300, grow_fraction=0.5).any())
    # a plain pass next to a weighted one: the records are those of accumulate()
    plain = contribution.ContributionScores(model, tracer)
    for b in batches:
        plain.accumulate(b)
    assert torch.equal(plain.scores, scorer.scores) and "weighted_sum" not in plain.result()

    changed = torch.zeros(300, dtype=torch.bool)
    changed[torch.randperm(300, generator=torch.Generator().manual_seed(3))[:30]] = True
    changed = changed.to(DEV)
    model.features[changed, 0:3] += 0.5
    scorer = contribution.ContributionScores(model, tracer)
    for b in batches:
        scorer.accumulate_error(b, "black")
    res = scorer.result()
    mean = torch.as_tensor(strategy.error_score_of(res, "error_mean"), device=DEV)
    seen = res["pixels"] > 0
    a, b = float(mean[seen & changed].median()), float(mean[seen & ~changed].median())
    print(f"[accumulate_error] {int((seen & changed).sum())} changed and {int((seen & ~changed).sum())} unchanged rows drawn: median "
          f"error_mean {a:.4f} vs {b:.4f}; {int((res['weighted_sum'] > 0).sum())} rows with an error")
    assert int((seen & changed).sum()) >= 10 and a > b
    assert bool((res["weighted_sum"] <= res["weight_sum"]).all())
    sel = strategy.select_by_error(res, 300, grow_fraction=0.1)
    assert int(sel.sum()) == 30 and bool((res["weighted_sum"][sel] > 0).all())
