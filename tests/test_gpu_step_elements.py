"""The stateless optimiser / activation entry points of the C ABI against tests/reference_step.py (float64), EVERY element of every
output, on inputs a random scene never produces: second moments from denormal to 1e20 (dense around the switch of the kernels' square
root at 2^-96 and around 2^-126), cancelling first moments, zero rows, parameters that are exactly 0, logits from -100 to 89,
log-scales from -20 to 10, quaternion norms from 1e-20 to 1e6, steps 0 ... 1e6, two eps, all learning-rate columns different, row
counts with partial waves and partial 256-row blocks.

The tolerance of an element is reference_step's Cond.bound(K) — derived shape, one constant per family measured on the CPU
(tests/common.py, tests/test_cpu_reference_step.py).  No element is excluded from any comparison.  Two documented behaviours are not
numbers to compare and are therefore not drawn: the chain rule below normalize's clamp (|q| < 1e-12) does not occur in these
entry points at all, and no Gaussian sits exactly on a camera position (its direction is 0 / 0).
Each case prints `[elements <case>] worst = <ratio> of bound`."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import reference_step as R
from tests.common import K_ACT, K_ADAM, K_ADAM_IEEE, K_CHAIN, K_MOMENT

pytestmark = pytest.mark.gpu
capi = importlib.import_module("3dgrut_amd._capi")

B1, B2 = 0.9, 0.999
DEV = "cuda:0"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _fa(a):
    a = np.asarray(a, np.float32)
    return (C.c_float * a.size)(*a.tolist())


def _ptr(t, row0=0):
    """device pointer of row `row0` of a contiguous 2-D (or 1-D) tensor, or None"""
    if t is None:
        return None
    return t.data_ptr() + row0 * (t.stride(0) if t.dim() > 1 else 1) * t.element_size()


class Worst:
    def __init__(self, case):
        self.case, self.worst, self.where, self.used = case, 0.0, "", None

    def check(self, what, got, ref, bound):
        """every element: |got - ref| <= bound (bound == 0: equal).  No exclusions.  bound = (Cond, K): the bound is cond.bound(K), and
        the share of K the worst element used, (|difference| - non-scaling terms) / (EPS S), is recorded for the report."""
        cond = None
        if isinstance(bound, tuple):
            cond, K = bound
            bound = cond.bound(K)
        got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64).reshape(np.shape(ref))
        ref = np.asarray(ref, np.float64); bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
        assert np.isfinite(ref).all() and np.isfinite(bound).all(), f"{self.case}/{what}: the reference is not finite"
        assert np.isfinite(got).all(), f"{self.case}/{what}: {int((~np.isfinite(got)).sum())} non-finite elements, first at {np.argwhere(~np.isfinite(got))[0]}"
        err = np.abs(got - ref)
        if cond is not None and (cond.rel > 0).any():
            self.used = max(self.used or 0.0, float((np.maximum(err - cond.abs, 0.0)[cond.rel > 0] / (R.EPS * cond.rel[cond.rel > 0])).max()))
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
        w = float(ratio[k]) if ratio.size else 0.0
        if w > self.worst:
            self.worst, self.where = w, f"{what}{list(map(int, k))}"
        assert w <= 1.0, (f"{self.case}/{what}: {int((ratio > 1).sum())} of {ratio.size} elements outside their bound; worst at {list(map(int, k))}: "
                          f"gpu {got[k]!r} reference {ref[k]!r} |difference| {err[k]:.3e} bound {bound[k]:.3e} ({w:.2f} x)")

    def bits(self, what, got, want):
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
        same = got.view(np.uint32) == want.view(np.uint32) if got.dtype == np.float32 else got == want
        assert same.all(), f"{self.case}/{what}: {int((~same).sum())} elements changed bits, first at {np.argwhere(~same)[0]}"

    def report(self):
        used = "" if self.used is None else f"; largest (|difference| - half ulp and input terms) / (EPS S) = {self.used:.2f}"
        print(f"[elements {self.case}] worst = {self.worst:.3f} of bound ({self.where}){used}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. gut_activate_pack
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_activate_pack_every_element(n):
    lib = capi.load()
    raw = R.draw_raw_rows(n, 100 + n)
    d_raw = _dev(raw); d_act = torch.full((n, 12), float("nan"), device=DEV)
    assert lib.gut_activate_pack(_stream(), n, d_raw.data_ptr(), d_act.data_ptr()) == 0
    ref, cond = R.activate(raw)
    w = Worst(f"activate_pack N={n}")
    w.check("act12", d_act, ref, (cond, K_ACT))
    w.bits("positions", d_act[:, :3], raw[:, :3])
    w.report()


def test_activate_pack_sigmoid_is_monotone_and_finite_at_the_extremes():
    lib = capi.load()
    n = 100000
    x = np.sort(np.concatenate([np.linspace(-104.0, 92.0, n - 2 * len(R.EXTREME_LOGITS)), R.EXTREME_LOGITS, R.EXTREME_LOGITS]).astype(np.float32))
    raw = np.zeros((n, 12), np.float32); raw[:, 3] = x; raw[:, 4] = 1.0
    raw[::7, 4] = 0.0                                          # the zero quaternion among them
    d_act = torch.full((n, 12), float("nan"), device=DEV)
    assert lib.gut_activate_pack(_stream(), n, _dev(raw).data_ptr(), d_act.data_ptr()) == 0
    act = d_act.cpu().numpy()
    assert np.isfinite(act).all()
    y = act[:, 3].astype(np.float64)
    assert (np.diff(y) >= 0).all(), f"sigmoid decreases at logit {x[1:][np.diff(y) < 0][:3]}"
    assert y.min() >= 0.0 and y.max() <= 1.0 and y[x == 0][0] == 0.5
    ref, cond = R.activate(raw)
    w = Worst("activate_pack sweep")
    w.check("act12", act, ref, (cond, K_ACT))
    w.report()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. gut_adam_step (IEEE form) and gut_selective_adam
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cols", [(1, 4), (63, 12), (257, 48), (1000, 64), (4097, 12), (100003, 48)])
def test_adam_step_every_element(n, cols):
    lib = capi.load()
    w = Worst(f"adam_step N={n} C={cols}")
    lr = R.lr_ladder(cols)
    steps = R.STEPS if n <= 4097 else (0, 1, 1024)
    for j, step in enumerate(steps):
        eps = (1e-15, 1e-8)[j % 2]
        p, g, m, v = R.draw_adam_inputs(n, cols, 7 * n + step % 1000)
        vis = None
        if step == 0:                                         # SelectiveAdam semantics: float mask, masked rows untouched
            vis = (np.random.default_rng(n).random(n) < 0.6).astype(np.float32)
        dp, dg, dm, dv = _dev(p), _dev(g), _dev(m), _dev(v)
        dvis = None if vis is None else _dev(vis)
        assert lib.gut_adam_step(_stream(), n, cols, dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), _fa(lr), B1, B2, eps, step,
                                 _ptr(dvis)) == 0
        (rp, rm, rv), (cp, cm, cv) = R.adam(p, g, m, v, lr, B1, B2, eps, step, visibility=vis)
        w.check(f"p(step {step})", dp, rp, (cp, K_ADAM_IEEE)); w.check(f"m(step {step})", dm, rm, (cm, K_MOMENT)); w.check(f"v(step {step})", dv, rv, (cv, K_MOMENT))
        w.bits("gradient untouched", dg, g)
    w.report()


@pytest.mark.parametrize("cols", [1, 3, 4, 45])
def test_selective_adam_every_element(cols):
    lib = capi.load()
    w = Worst(f"selective_adam C={cols}")
    for n, eps in ((1, 1e-15), (65, 1e-8), (257, 1e-15), (4097, 1e-8)):
        p, g, m, v = R.draw_adam_inputs(n, cols, 31 * n + cols)
        vis = np.random.default_rng(n + cols).random(n) < 0.5
        lr = float(np.float32(3e-3))
        dp, dg, dm, dv, dvis = _dev(p), _dev(g), _dev(m), _dev(v), _dev(vis)
        assert dvis.dtype == torch.bool
        assert lib.gut_selective_adam(_stream(), n, cols, dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), dvis.data_ptr(), lr, B1, B2, eps) == 0
        (rp, rm, rv), (cp, cm, cv) = R.adam(p, g, m, v, np.full(cols, lr, np.float32), B1, B2, eps, 0, visibility=vis)
        w.check("p", dp, rp, (cp, K_ADAM_IEEE)); w.check("m", dm, rm, (cm, K_MOMENT)); w.check("v", dv, rv, (cv, K_MOMENT))
    w.report()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. - 6. the fused step
# ---------------------------------------------------------------------------------------------------------------------------------
CAMERAS = np.array([[0.5, -1.0, -4.0], [3.0, 0.2, 1.0], [-2.0, 2.5, 0.3], [0.0, 0.0, 9.0], [1.0, 1.0, 1.0]], np.float32)
LR12, LR48 = R.lr_ladder(12), R.lr_ladder(48, 2e-5, 3e-2)


class FusedCase:
    """Inputs of one fused step (numpy, fp32) and their device copies."""

    def __init__(self, n, seed, views=1, stride=0, degree=3):
        rng = np.random.default_rng(seed)
        self.n, self.views, self.degree = n, views, degree
        self.stride = stride if stride else n
        self.cams = CAMERAS[:views].copy()
        p12, self.g12, self.m12, self.v12 = R.draw_adam_inputs(n, 12, seed + 1)
        self.sh48, _, self.m48, self.v48 = R.draw_adam_inputs(n, 48, seed + 2)
        raw = R.draw_raw_rows(n, seed + 3)
        raw[:, 0:3] = p12[:, 0:3]; raw[:, 11] = p12[:, 11]      # positions and the unused column from the parameter table (exact zeros included)
        c0 = self.cams[0].astype(np.float64); u = np.array([0.6, -0.48, 0.64])
        if n > 2:
            raw[0, 0:3] = c0 + 1e-3 * u; raw[1, 0:3] = c0 + 1e4 * u
        on_camera = (raw[:, None, 0:3] == self.cams[None]).all(-1).any(1)
        raw[on_camera, 0] += 1.0                               # (no Gaussian exactly at a camera position)
        self.raw = raw
        # compact per-view dL/dRGB rows: zero wherever the raw gradient row is zero (a Gaussian without a gradient has none in any view),
        # and zero in some views of the others
        mr = rng.choice([-1.0, 1.0], (views, self.stride, 3)) * np.exp(rng.uniform(np.log(1e-12), np.log(1e3), (views, self.stride, 3)))
        mr[rng.random((views, self.stride)) < 0.3] = 0.0
        if n > 2:   # the two rows placed 1e-3 and 1e+4 from camera 0 always have a gradient and a dL/dRGB in view 0: the case never rests on a seed
            self.g12[:2, :11] = np.where(self.g12[:2, :11] == 0, np.float32(0.37), self.g12[:2, :11])
            mr[0, :2] = np.where(mr[0, :2] == 0, 0.83, mr[0, :2])
        zero_row = ~self.g12[:, :11].any(1)
        mr[:, :n][:, zero_row] = 0.0
        self.mrgb = mr.astype(np.float32)
        self.g12[:, 11] = 0.0

    def device(self):
        return {k: _dev(getattr(self, k)) for k in ("raw", "m12", "v12", "sh48", "m48", "v48", "g12", "mrgb", "cams")}

    def launch(self, lib, d, step, eps, grad_scale, r0=0, r1=None, vis=None, act=None, flags=0, wave_flags=None, lazy=None, reg=None):
        r1 = self.n if r1 is None else r1
        rc = lib.gut_sh_adam_step_regularised(
            _stream(), r1 - r0, self.degree, self.views, d["cams"].data_ptr(), d["mrgb"].data_ptr() + r0 * 12, _ptr(d["g12"], r0),
            grad_scale, _ptr(d["raw"], r0), _ptr(d["m12"], r0), _ptr(d["v12"], r0), _ptr(d["sh48"], r0), _ptr(d["m48"], r0), _ptr(d["v48"], r0),
            _fa(LR12), _fa(LR48), B1, B2, eps, step, _ptr(vis, r0), _ptr(act, r0), 0 if self.stride == self.n and r0 == 0 and r1 == self.n else self.stride,
            flags, _ptr(wave_flags, r0 // 64), lazy, reg)
        assert rc == 0, rc

    def reference(self, step, eps, grad_scale, vis=None, reg=None):
        return R.step(self.raw, self.m12, self.v12, self.sh48, self.m48, self.v48, self.g12, self.cams, self.mrgb[:, :self.n], self.degree,
                      grad_scale, LR12, LR48, B1, B2, eps, step, visibility=vis, reg=reg)


KEYS = (("raw", "raw12", K_ADAM), ("m12", "m12", K_MOMENT), ("v12", "v12", K_MOMENT), ("sh48", "sh48", K_ADAM), ("m48", "m48", K_MOMENT),
        ("v48", "v48", K_MOMENT))      # the parameters: the fast-math constant; the moments: their own, tighter one


def _check_step(w, d, act, ref, tag="", vis=None):
    """vis: the visibility mask the step was given (None: every row was updated).  The activated rows of masked rows are compared by
    the caller with what it had put there; every other row of act12 is compared here — selected by the mask, not by the reference."""
    for key, name, K in KEYS:
        val, cond = ref[name]
        w.check(name + tag, d[key], val, (cond, K))
    if act is not None:
        val, cond = ref["act12"]
        on = np.ones(val.shape[0], bool) if vis is None else (np.asarray(vis).reshape(-1) != 0)
        w.check("act12" + tag, act[torch.as_tensor(on, device=DEV)], val[on], cond.bound(0.0)[on])


def _fused_configs(n):
    """(step, eps, views, stride, grad_scale, degree): every value of the issue's table occurs, and every (views, degree) pair; all ten step values at
    N = 1000 (ten configurations, not a cross product), three at the other sizes, two at N = 100 003."""
    idx = R.SIZES.index(n)
    steps = R.STEPS if n == 1000 else tuple(R.STEPS[(idx + 3 * j) % len(R.STEPS)] for j in range(3 if n <= 4097 else 2))
    out = []
    for j, step in enumerate(steps):
        views = (1, 2, 5)[(idx + j) % 3]
        out.append((step, (1e-15, 1e-8)[(idx + j) % 2], views, (0, n + 7)[(idx // 2 + j) % 2], (1.0, 1.0 / views)[(idx + j // 2) % 2], (3, 0, 1, 2)[(idx + j) % 4]))
    return out


@pytest.mark.parametrize("n", R.SIZES)
def test_fused_step_every_element(n):
    """gut_sh_adam_step_regularised without regulariser, lazy moments or flags: the fast-math Adam form, the SH-gradient rebuild with
    its LDS transpose, and the activated row it writes, against reference_step.step."""
    lib = capi.load()
    w = Worst(f"fused step N={n}")
    for step, eps, views, stride, gs, degree in _fused_configs(n):
        case = FusedCase(n, 1000 * n + step % 997, views, stride, degree)
        d = case.device()
        act = torch.full((n, 12), float("nan"), device=DEV)
        case.launch(lib, d, step, eps, gs, act=act)
        ref = case.reference(step, eps, gs)
        _check_step(w, d, act, ref, f"(step {step} V={views} deg={degree} stride={stride} gs={gs:.2g} eps={eps:g})")
        w.bits("gradient rows untouched", d["g12"], case.g12); w.bits("mrgb untouched", d["mrgb"], case.mrgb)
    w.report()


@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_fused_step_with_a_visibility_mask_leaves_masked_rows_alone(n):
    lib = capi.load()
    w = Worst(f"fused step, visibility mask, N={n}")
    case = FusedCase(n, 77 + n, views=2, stride=n + 7, degree=3)
    d = case.device()
    vis = (np.random.default_rng(n).random(n) < 0.5).astype(np.float32)
    if n > 64:
        vis[64:128] = 0.0                                       # a whole wave masked
    act0 = np.random.default_rng(n + 1).normal(size=(n, 12)).astype(np.float32)
    act = _dev(act0)
    case.launch(lib, d, 0, 1e-15, 0.5, vis=_dev(vis), act=act)
    ref = case.reference(0, 1e-15, 0.5, vis=vis)
    _check_step(w, d, act, ref, vis=vis)
    off = torch.as_tensor(vis == 0, device=DEV)
    for key in ("raw", "m12", "v12", "sh48", "m48", "v48"):
        w.bits(key + " of masked rows", d[key][off], getattr(case, key)[vis == 0])
    w.bits("act12_out of masked rows", act[off], act0[vis == 0])
    w.report()


def test_clear_consumed_grads_wave_flags_and_row_ranges():
    """GUT_ADAM_CLEAR_CONSUMED_GRADS zeroes exactly the rows it read as non-zero; d_wave_flags leaves flag-0 waves bit-unchanged; the
    union of row-range calls [r0, r1) (r0 a multiple of 256, the last ending in a partial wave) equals one call, bit for bit."""
    lib = capi.load()
    n = 4097 + 300
    w = Worst("fused step: clear / wave flags / row ranges")
    case = FusedCase(n, 4242, views=2, stride=n + 7, degree=3)
    keys = ("raw", "m12", "v12", "sh48", "m48", "v48")
    # one call
    d1 = case.device(); act1 = torch.full((n, 12), -7.0, device=DEV)
    case.launch(lib, d1, 5, 1e-15, 0.5, act=act1)
    ref = case.reference(5, 1e-15, 0.5)
    _check_step(w, d1, act1, ref)
    # chunks of 1024 rows + a tail, with the clear flag
    d2 = case.device(); act2 = torch.full((n, 12), -7.0, device=DEV)
    for r0 in range(0, n, 1024):
        case.launch(lib, d2, 5, 1e-15, 0.5, r0=r0, r1=min(n, r0 + 1024), act=act2, flags=capi.ADAM_CLEAR_CONSUMED_GRADS)
    for k in keys:
        w.bits(k + " chunked == one call", d2[k], d1[k])
    w.bits("act12 chunked == one call", act2, act1)
    assert not d2["g12"].any(), "consumed gradient rows are not zero"
    assert not d2["mrgb"][:, :n].any(), "consumed dL/dRGB rows are not zero"
    w.bits("mrgb padding rows untouched", d2["mrgb"][:, n:], case.mrgb[:, n:])
    # wave flags: flag-0 waves untouched (gradient rows included, clear flag or not), the others as in the one call
    waves = (n + 63) // 64
    flags = (np.random.default_rng(3).random(waves) < 0.5).astype(np.uint8); flags[-1] = 1; flags[0] = 0
    rows_on = np.repeat(flags, 64)[:n].astype(bool)
    d3 = case.device(); act3 = torch.full((n, 12), -7.0, device=DEV)
    case.launch(lib, d3, 5, 1e-15, 0.5, act=act3, flags=capi.ADAM_CLEAR_CONSUMED_GRADS, wave_flags=_dev(flags))
    on, off = torch.as_tensor(rows_on, device=DEV), torch.as_tensor(~rows_on, device=DEV)
    for k in keys:
        w.bits(k + " of walked waves", d3[k][on], d1[k][on])
        w.bits(k + " of skipped waves", d3[k][off], getattr(case, k)[~rows_on])
    w.bits("act12 of walked waves", act3[on], act1[on]); assert (act3[off] == -7.0).all()
    w.bits("gradient rows of skipped waves", d3["g12"][off], case.g12[~rows_on]); assert not d3["g12"][on].any()
    w.bits("mrgb of skipped waves", d3["mrgb"][:, :n][:, off], case.mrgb[:, :n][:, ~rows_on]); assert not d3["mrgb"][:, :n][:, on].any()
    w.report()


# ---- 5. lazy moments ------------------------------------------------------------------------------------------------------------
def _lazy(n, table_len):
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    t = dict(wave_step=torch.zeros((n + 63) // 64, dtype=torch.int32, device=DEV),
             pow1=_dev((b1 ** np.arange(table_len)).astype(np.float32)), pow2=_dev((b2 ** np.arange(table_len)).astype(np.float32)),
             overrun=torch.zeros(1, dtype=torch.int32, device=DEV))
    t["struct"] = capi.GutLazyMoments(t["wave_step"].data_ptr(), t["pow1"].data_ptr(), t["pow2"].data_ptr(), table_len, t["overrun"].data_ptr())
    return t


def _unwalked(lib, case, d, flags, step, eps, act, lazy=None, reg=None):
    rc = lib.gut_adam_unwalked_waves_regularised(_stream(), case.n, flags.data_ptr(), d["raw"].data_ptr(), d["m12"].data_ptr(), d["v12"].data_ptr(),
                                                 d["sh48"].data_ptr(), d["m48"].data_ptr(), d["v48"].data_ptr(), _fa(LR12), _fa(LR48), B1, B2, eps,
                                                 step, _ptr(act), lazy, reg)
    assert rc == 0, rc


@pytest.mark.parametrize("k,n", [(1, 4097), (2, 257), (7, 1000), (500, 257), (1023, 321)])
def test_lazy_moments_against_eager_float64_steps(k, n):
    """k zero-gradient steps through gut_adam_unwalked_waves_ex with a GutLazyMoments (moments read, decayed in registers, never
    stored), one step with a gradient on the walked half of the waves (the other half takes its zero-gradient step), then
    gut_sync_moments_ex: parameters AND synced moments against k + 1 eager float64 steps.  The lazy form's folded constants meet an
    outside reference here and nowhere else.  Bound: the per-step bound of every step added up (each step rounds the parameter), with
    K_ADAM + 2 (parameters) and K_MOMENT + 2 (moments) for the two extra roundings of the decay factor (the table entry beta^k, and its product with the stored moment), and
    the table's ABSOLUTE rounding step where beta1^k is denormal or zero in fp32 (0.9^k below 2^-126 from k = 829; (float) 0.9^1024 = 0):
    |stored moment| x 2^-149, pushed through the update with D >= eps."""
    lib = capi.load()
    eps = 1e-15
    w = Worst(f"lazy moments k={k} N={n}")
    case = FusedCase(n, 9000 + k, views=1, stride=0, degree=3)
    waves = (n + 63) // 64
    flags = (np.arange(waves) % 2 == 0).astype(np.uint8)
    rows_on = np.repeat(flags, 64)[:n].astype(bool)
    # the SH direction of step k + 1 comes from the position BEFORE that step: rows that will take the gradient get zero position
    # moments, so that their position stays bit-exact through the zero-gradient steps and the direction is the same on both sides
    # (the other rows keep theirs and move on their momentum)
    case.m12[rows_on, 0:3] = 0.0
    d = case.device()
    lz = _lazy(n, k + 3)
    act = torch.full((n, 12), float("nan"), device=DEV)
    all_unwalked = torch.zeros(waves, dtype=torch.uint8, device=DEV)
    for t in range(1, k + 1):
        _unwalked(lib, case, d, all_unwalked, t, eps, act, lazy=C.byref(lz["struct"]))
    assert int(lz["overrun"].item()) == 0 and not lz["wave_step"].any()
    w.bits("stored m12 untouched by lazy steps", d["m12"], case.m12); w.bits("stored v48 untouched by lazy steps", d["v48"], case.v48)
    dflags = _dev(flags)
    case.launch(lib, d, k + 1, eps, 1.0, act=act, wave_flags=dflags, lazy=C.byref(lz["struct"]))
    _unwalked(lib, case, d, dflags, k + 1, eps, act, lazy=C.byref(lz["struct"]))
    assert lib.gut_sync_moments_ex(_stream(), n, d["m12"].data_ptr(), d["v12"].data_ptr(), d["m48"].data_ptr(), d["v48"].data_ptr(),
                                   C.byref(lz["struct"]), k + 1, None) == 0
    torch.cuda.synchronize()
    assert int(lz["overrun"].item()) == 0 and (lz["wave_step"] == k + 1).all()
    # k + 1 eager float64 steps
    st = {"12": [case.raw.astype(np.float64), case.m12.astype(np.float64), case.v12.astype(np.float64)],
          "48": [case.sh48.astype(np.float64), case.m48.astype(np.float64), case.v48.astype(np.float64)]}
    g_last = {"12": np.where(rows_on[:, None], case.g12.astype(np.float64), 0.0),
              "48": np.where(rows_on[:, None], R.sh_gradient(case.raw[:, :3], case.cams, case.mrgb[:, :n], 3, 1.0)[0], 0.0)}
    unc_last = {"12": None, "48": np.where(rows_on[:, None], R.sh_gradient(case.raw[:, :3], case.cams, case.mrgb[:, :n], 3, 1.0)[1], 0.0)}
    total = {"12": 0.0, "48": 0.0}
    conds = {}
    for t in range(1, k + 2):
        for blk, lr in (("12", LR12), ("48", LR48)):
            p, m, v = st[blk]
            g = g_last[blk] if t == k + 1 else np.zeros_like(p)
            (p, m, v), (cp, cm, cv) = R.adam(p, g, m, v, lr, B1, B2, eps, t, g_unc=unc_last[blk] if t == k + 1 else None)
            st[blk] = [p, m, v]
            table_step = R.DENORM_STEP * np.abs({"12": case.m12, "48": case.m48}[blk].astype(np.float64))
            total[blk] = total[blk] + cp.bound(K_ADAM + 2) + (lr.astype(np.float64)[None, :] / 0.1) * table_step / float(np.float32(eps))
            conds[blk] = (R.Cond(cm.rel, cm.abs + table_step + 2 * R.DENORM_STEP), R.Cond(cv.rel, cv.abs + 2 * R.DENORM_STEP))
    for blk, pk, mk, vk in (("12", "raw", "m12", "v12"), ("48", "sh48", "m48", "v48")):
        w.check(pk, d[pk], st[blk][0], total[blk])
        w.check(mk, d[mk], st[blk][1], conds[blk][0].bound(K_MOMENT + 2))
        w.check(vk, d[vk], st[blk][2], conds[blk][1].bound(K_MOMENT + 2))
    aref, acond = R.activate(st["12"][0], raw_unc=total["12"])
    w.check("act12", act, aref, acond.bound(K_ACT))
    w.report()


def test_lazy_overrun_word():
    """A wave whose stored moments have missed table_len steps has no decay factor in the tables: the overrun word stays 0 through
    table_len zero-gradient steps and is 1 after the next call (no result is asserted for that call)."""
    lib = capi.load()
    n, L = 130, 8
    case = FusedCase(n, 5, views=1)
    d = case.device()
    lz = _lazy(n, L)
    flags = torch.zeros((n + 63) // 64, dtype=torch.uint8, device=DEV)
    for t in range(1, L + 1):
        _unwalked(lib, case, d, flags, t, 1e-15, None, lazy=C.byref(lz["struct"]))
        assert int(lz["overrun"].item()) == 0, t
    _unwalked(lib, case, d, flags, L + 1, 1e-15, None, lazy=C.byref(lz["struct"]))
    assert int(lz["overrun"].item()) == 1


# ---- 6. the regularisers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_regularised_entry_points_every_element(n):
    lib = capi.load()
    w = Worst(f"regularisers N={n}")
    dc, sc = 1e-3, 1e-4
    waves = (n + 63) // 64
    case = FusedCase(n, 600 + n, views=2, stride=n + 7, degree=2)
    rg, rcond, rpart = R.regulariser(case.raw, dc, sc)
    pbound = 64 * R.EPS * np.abs(rpart) + 64 * R.FLT_MIN_NORMAL     # (+ the fp32 sigmoid's underflow below logit -87.3, per row of the wave)

    def reg_struct():
        part = torch.full((waves, 2), float("nan"), device=DEV)
        return part, capi.GutRegularisation(dc, sc, part.data_ptr())

    # (a) gut_regularisation_gradient: adds the two terms into a materialised raw gradient
    part, rs = reg_struct()
    dg = _dev(case.g12)
    assert lib.gut_regularisation_gradient(_stream(), n, _dev(case.raw).data_ptr(), dg.data_ptr(), C.byref(rs)) == 0
    total = case.g12.astype(np.float64) + rg
    w.check("gradient + regulariser", dg, total, rcond.bound(K_CHAIN) + 0.5 * R.ulp32_up(np.abs(total) + rcond.bound(K_CHAIN)))
    w.bits("untouched gradient columns", dg[:, [0, 1, 2, 4, 5, 6, 7, 11]], case.g12[:, [0, 1, 2, 4, 5, 6, 7, 11]])
    w.check("partials (gradient)", part, rpart, pbound)
    # (b) the fused step with the regulariser
    for step, eps, gs in ((1, 1e-15, 1.0), (1000, 1e-8, 0.5)):
        part, rs = reg_struct()
        d = case.device(); act = torch.full((n, 12), float("nan"), device=DEV)
        case.launch(lib, d, step, eps, gs, act=act, reg=C.byref(rs))
        _check_step(w, d, act, case.reference(step, eps, gs, reg=(dc, sc)), f"(regularised, step {step})")
        w.check("partials (fused step)", part, rpart, pbound)
    # (c) the zero-gradient pass with the regulariser on the flag-0 waves; the other waves bit-unchanged
    flags = (np.arange(waves) % 2 == 1).astype(np.uint8)
    rows_off = ~np.repeat(flags, 64)[:n].astype(bool)
    part, rs = reg_struct()
    d = case.device(); act = torch.full((n, 12), -7.0, device=DEV)
    _unwalked(lib, case, d, _dev(flags), 10, 1e-15, act, reg=C.byref(rs))
    zero = FusedCase(n, 600 + n, views=2, stride=n + 7, degree=2)
    zero.g12[:] = 0.0; zero.mrgb[:] = 0.0
    ref = zero.reference(10, 1e-15, 1.0, reg=(dc, sc))
    sel = torch.as_tensor(rows_off, device=DEV)
    for key, name, K in KEYS:
        val, cond = ref[name]
        w.check(name + "(zero-gradient pass)", d[key][sel], val[rows_off], cond.bound(K)[rows_off])
        w.bits(key + " of walked waves", d[key][~sel], getattr(case, key)[~rows_off])
    val, cond = ref["act12"]
    w.check("act12(zero-gradient pass)", act[sel], val[rows_off], cond.bound(0.0)[rows_off]); assert (act[~sel] == -7.0).all()
    w.check("partials (zero-gradient pass)", part[torch.as_tensor(flags == 0, device=DEV)], rpart[flags == 0], pbound[flags == 0])
    w.report()
