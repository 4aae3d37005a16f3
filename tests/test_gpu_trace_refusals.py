"""A refused backward leaves the handle as it was, for each of the five backward forms (trace_bwd, trace_bwd with skip_epilogue,
trace_bwd_fields, trace_bwd_model_fields, trace_bwd_pose) at N = 257 (one 256-row block plus one row) and 37 x 53 pixels (partial
edge tiles).  On one handle the backward is refused four ways — no forward yet, a *_fields backward (pose: an int N) after a forward
that was given packed rows, the wrong N, the wrong resolution — each with the library's own message and nothing queued; then the
matching backward runs and its results are compared with those of a handle that was never refused anything.

"Nothing queued" is observed through the tensors a backward would write: the pose output every backward reduces into while one is
set (set_pose_gradient; it keeps its sentinel) and, where the form takes them, the caller's gradient tensors (`out=`).

The comparison: the zero pattern of every result equals the untouched handle's, and every result differs from it by at most twice
what two runs of the untouched handle differ from each other, measured here from two such runs.  The gradient rows accumulate with
float atomics, whose order is not fixed; the upstream gradient is non-zero in two pixels of two different tiles only, so every
accumulator receives at most two non-zero terms (one per tile; a pixel's terms are reduced inside its wave in a fixed order, every
other term is an exact zero) and their sum does not depend on the order.  The two reference runs therefore agree to the bit, and so
must the handle under test: the bound stays twice the measured spread, the inputs make it a sharp one."""
import importlib
import re

import numpy as np
import pytest
import torch

from tests.common import cams, make_view, scenes, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
DEV = "cuda:0"
N, W, H = 257, 37, 53
FORMS = ("rows", "rows_skip", "fields", "model_fields", "pose")

NO_FORWARD = "gut_trace_bwd: no forward context on this stream (call gut_trace first, same stream)"
NO_PACKED = {
    "fields": "gut_trace_bwd_fields: no gut_trace_fields forward on this handle",
    "model_fields": "gut_trace_bwd_model_fields: no gut_trace_fields / gut_trace_model_fields forward on this handle",
    "pose": "gut_trace_bwd_pose: d_particle_density is NULL and the last forward on this handle packed no rows (not a *_fields one)",
}


def _differ(n, w, h):
    return f"gut_trace_bwd: arguments differ from the cached forward (N {n} vs {N}, {w}x{h} vs {W}x{H})"


def _view(w, h):
    view = make_view("pinhole", w, h, cams.look_at_c2w((0.3, -0.2, -4.0), (0, 0, 0)), fx=1.1 * w)
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    up = torch.zeros((h, w, 5), dtype=torch.float32, device=DEV)   # [..., :4] the rgba gradient, [..., 4:] the hit-distance gradient
    # two pixels under the middle of the scene (the CPU oracle counts 22 and 16 hits there at 37 x 53), in the tiles (0,1) and (1,1)
    for (y, x), g in (((25, 10), (0.7, -1.1, 0.4, 0.9, 0.3)), ((26, 21), (-0.5, 0.8, 1.2, -0.6, -0.2))):
        up[y, x] = torch.tensor(g, device=DEV)
    return dict(ro=ro, rd=rd, tail=(sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1]),
                rgba_g=up[..., :4].contiguous(), dist_g=up[..., 4:].contiguous())


@pytest.fixture(scope="module")
def setup():
    sc = scenes.scene_c1(N, 11)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    d12, sph = scenes.pack_density(sc), sc["features"].astype(np.float32)
    T = dict(d12=t(d12), sph=t(sph), pos=t(d12[:, 0:3]), dns=t(d12[:, 3:4]), rot=t(d12[:, 4:8]), scl=t(d12[:, 8:11]), alb=t(sph[:, 0:3]),
             spec=t(sph[:, 3:48]))
    return T, _view(W, H), _view(40, 56)


def _handle():
    raster = gut.Tracer({"render": {}}).tracer_wrapper
    out8 = torch.full((8,), 7.0, dtype=torch.float32, device=DEV)
    raster.set_pose_gradient(out8)
    return raster, out8


def _forward(form, raster, T, v):
    if form in ("rows", "rows_skip"):
        return raster.trace(0, 3, T["d12"], T["sph"], v["ro"], v["rd"], None, *v["tail"])
    if form == "model_fields":
        return raster.trace_model_fields(0, 3, T["pos"], T["dns"], T["rot"], T["scl"], T["alb"], T["spec"], v["ro"], v["rd"], *v["tail"])
    return raster.trace_fields(0, 3, T["pos"], T["dns"], T["rot"], T["scl"], T["sph"], v["ro"], v["rd"], *v["tail"])


def _backward(form, raster, T, v, rgba, dist, n=N, out=None):
    """The form's backward for n rows of the view v; returns its result tensors (without the pose output)."""
    up = (rgba, v["rgba_g"], dist, v["dist_g"])
    if form == "rows":
        return list(raster.trace_bwd(0, 3, T["d12"][:n], T["sph"][:n], v["ro"], v["rd"], None, *v["tail"], *up, out=out))
    if form == "rows_skip":
        raster.trace_bwd(0, 3, T["d12"][:n], T["sph"][:n], v["ro"], v["rd"], None, *v["tail"], *up, skip_epilogue=True)
        return [raster.debug_buffer("grad_scratch")]    # the handle's gradient rows, left for optimize_after_bwd
    if form == "fields":
        return list(raster.trace_bwd_fields(0, 3, n, T["sph"][:n], v["ro"], v["rd"], *v["tail"], *up))
    if form == "model_fields":
        return list(raster.trace_bwd_model_fields(0, 3, n, v["ro"], v["rd"], *v["tail"], *up, out=out))
    raster.trace_bwd_pose(0, 3, n, v["ro"], v["rd"], *v["tail"], *up)   # int N: the rows the *_fields forward packed
    return [raster.debug_buffer("grad_scratch")]        # no per-Gaussian output: the reduction leaves the handle's rows zero


def _untouched(form, T, v):
    raster, out8 = _handle()
    rgba, dist, _, _ = _forward(form, raster, T, v)
    res = _backward(form, raster, T, v, rgba, dist) + [out8]
    torch.cuda.synchronize()
    return [r.clone() for r in res]


def _sentinels(form):
    if form == "rows":
        return tuple(torch.full((N, c), 7.0, dtype=torch.float32, device=DEV) for c in (12, 48))
    if form == "model_fields":
        return tuple(torch.full((N, c), 7.0, dtype=torch.float32, device=DEV) for c in (3, 1, 4, 3, 3, 45))
    return None


@pytest.mark.parametrize("form", FORMS)
def test_refused_backward_leaves_the_handle_as_it_was(form, setup):
    T, v, other = setup
    ref1, ref2 = _untouched(form, T, v), _untouched(form, T, v)
    assert any(bool(r.any()) for r in ref1[:-1]) or form == "pose", "the reference backward produced no gradient at all"
    assert bool(ref1[-1][:6].any()), "the reference backward produced no pose gradient"

    raster, out8 = _handle()
    keep = _sentinels(form)

    def refused(message, call):
        with pytest.raises(RuntimeError, match=re.escape(message)):
            call()
        torch.cuda.synchronize()
        assert out8.tolist() == [7.0] * 8, f"{message!r}: the refused backward wrote the pose output"
        assert keep is None or all(bool((k == 7.0).all()) for k in keep), f"{message!r}: the refused backward wrote a gradient tensor"

    blank = torch.zeros((H, W, 4), dtype=torch.float32, device=DEV), torch.zeros((H, W, 1), dtype=torch.float32, device=DEV)
    # 1. no forward on this handle yet (the pose form with the rows given: it needs no packed rows, only a forward)
    if form == "pose":
        refused(NO_FORWARD, lambda: raster.trace_bwd_pose(0, 3, T["d12"], v["ro"], v["rd"], *v["tail"], blank[0], v["rgba_g"], blank[1], None))
    else:
        refused(NO_PACKED.get(form, NO_FORWARD), lambda: _backward(form, raster, T, v, *blank, out=keep))
    # 2. a *_fields backward (pose: an int N) after a forward that was given packed rows
    rgba, dist, _, _ = raster.trace(0, 3, T["d12"], T["sph"], v["ro"], v["rd"], None, *v["tail"])
    packed_form = form if form in NO_PACKED else ("fields" if form == "rows" else "model_fields")
    refused(NO_PACKED[packed_form], lambda: _backward(packed_form, raster, T, v, rgba, dist, out=keep if packed_form == form else None))
    # the matching forward, then 3. the wrong N and 4. the wrong resolution
    rgba, dist, _, _ = _forward(form, raster, T, v)
    refused(_differ(N - 1, W, H), lambda: _backward(form, raster, T, v, rgba, dist, n=N - 1,
                                                    out=None if keep is None else tuple(k[:N - 1] for k in keep)))
    o_rgba, o_dist = torch.zeros((56, 40, 4), dtype=torch.float32, device=DEV), torch.zeros((56, 40, 1), dtype=torch.float32, device=DEV)
    refused(_differ(N, 40, 56), lambda: _backward(form, raster, T, other, o_rgba, o_dist, out=keep))
    # the handle still accepts the matching backward, with the untouched handle's results
    got = _backward(form, raster, T, v, rgba, dist) + [out8]
    torch.cuda.synchronize()
    assert len(got) == len(ref1)
    for i, (g, a, b) in enumerate(zip(got, ref1, ref2)):
        assert g.shape == a.shape and torch.equal(g == 0, a == 0), f"{form}: zero pattern of result {i}"
        spread = float((a - b).abs().max()) if a.numel() else 0.0
        diff = float((g - a).abs().max()) if a.numel() else 0.0
        print(f"[refusals {form}] result {i} {tuple(a.shape)}: max |value| {float(a.abs().max()) if a.numel() else 0.0:.3e}, "
              f"two untouched runs differ by {spread:.3e}, the refused handle by {diff:.3e}")
        assert diff <= 2.0 * spread, f"{form}: result {i} differs by {diff:.3e}, two untouched runs by {spread:.3e}"
    if form == "pose":
        assert not bool(got[0].any()), "the pose-only backward left gradient rows behind"
