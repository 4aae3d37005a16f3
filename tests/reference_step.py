"""A float64 restatement of one optimiser step, element by element, with the condition scale of every element.

Written from include/gut_hip.h (row layouts, what each entry point is documented to compute) and from the documented semantics of
torch.sigmoid / torch.nn.functional.normalize / torch.exp / torch.optim.Adam and the reference's SelectiveAdam — NOT from the
kernels.  tests/test_cpu_reference_step.py validates it against torch in float64 and measures the constants of its tolerance model;
tests/test_gpu_step_elements.py and tests/test_gpu_raw_path.py hold the kernels against it, every element.

Every function returns its value(s) in float64 together with a `Cond` per output: the tolerance of an element is

        cond.bound(K) = K x EPS x cond.rel + cond.abs               EPS = 2^-23

`rel` is the sum of the ABSOLUTE values of the terms the element is formed from (not the element's own magnitude: where two terms
cancel the result is small and its fp32 error is not), `abs` holds what does not scale with the measured constant: half an ulp of
the stored fp32 result, the format's underflow steps, and the uncertainty an INPUT of the operation already carried (pushed through
the operation's derivative).  K is K_ADAM, K_ACT or K_CHAIN of tests/common.py.

Inputs are fp32 tensors (what the kernels are given); hyper-parameters the kernels hold in fp32 (betas, eps, learning rates,
regulariser coefficients) are rounded to fp32 first, as the host code must do to pass them.
"""
import math

import numpy as np

from tests.common import K_ACT, K_ADAM, K_CHAIN

EPS = 2.0 ** -23
DENORM_STEP = 2.0 ** -149      # spacing of fp32 below 2^-126: an operation whose result lands there has this absolute step
FLT_MIN_NORMAL = 2.0 ** -126   # below it a result may be flushed (1 / (1 + inf) = 0 is the fp32 sigmoid of a logit below -88.73)
NORMALIZE_EPS = 1e-12          # torch.nn.functional.normalize's default eps


class Cond:
    """Condition of an output: tolerance = K x EPS x rel + abs, per element."""

    def __init__(self, rel, abs_=0.0):
        self.rel = np.array(rel, np.float64)
        self.abs = np.broadcast_to(np.asarray(abs_, np.float64), self.rel.shape).copy()

    def bound(self, K):
        return K * EPS * self.rel + self.abs

    def rows(self, sel):
        return Cond(self.rel[sel], self.abs[sel])


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def ulp32_up(x):
    """fp32 spacing at |x|, taken one step up so that a result rounded across a binade boundary is covered."""
    a = np.abs(np.asarray(x, np.float64)) * (1.0 + 2.0 ** -22)
    with np.errstate(over="ignore"):
        return np.spacing(a.astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# activations  (gut_hip.h: raw row pos3 | density logit | quat4 | log-scale3 | unused  ->  pos3 | sigmoid | quat / |quat| | exp | |quat|)
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def activate(raw12, raw_unc=None):
    """raw12 [N,12] -> (act12 [N,12] float64, Cond).  raw_unc [N,12] (optional): an absolute uncertainty the raw row already carries
    (the optimiser's bound on the row it has just written); it is pushed through the activation's derivative into cond.abs."""
    raw = np.asarray(raw12, np.float64).reshape(-1, 12)
    n = raw.shape[0]
    act = np.zeros((n, 12)); rel = np.zeros((n, 12)); ab = np.zeros((n, 12))
    act[:, 0:3] = raw[:, 0:3]                                  # positions: copied, exact
    x = raw[:, 3]
    y = _sigmoid64(x)
    act[:, 3] = y
    rel[:, 3] = y
    # the relative error of expf: K_ACT EPS, plus EPS |x| for an expf that forms x log2(e) in fp32 (exp2 of a product rounded once;
    # the compiler's expansion of expf under floating-point contraction is such a form, see DESIGN.md par. 3);
    # d y / d(e^-x) x e^-x = -y (1 - y)
    ab[:, 3] = EPS * np.abs(x) * y * (1.0 - y) + FLT_MIN_NORMAL
    q = raw[:, 4:8]
    nq = np.sqrt((q * q).sum(1))
    nc = np.maximum(nq, NORMALIZE_EPS)
    qh = q / nc[:, None]
    act[:, 4:8] = qh
    rel[:, 4:8] = np.abs(qh)
    ab[:, 4:8] = DENORM_STEP
    s = raw[:, 8:11]
    act[:, 8:11] = np.exp(s)
    rel[:, 8:11] = np.exp(s)
    ab[:, 8:11] = EPS * np.abs(s) * np.exp(s) + DENORM_STEP     # the same expf term as in the sigmoid
    act[:, 11] = nc
    rel[:, 11] = nc
    if raw_unc is not None:
        u = np.asarray(raw_unc, np.float64).reshape(-1, 12)
        ab[:, 0:3] += u[:, 0:3]
        ab[:, 3] += y * (1.0 - y) * u[:, 3] + 0.5 * u[:, 3] ** 2       # |y''| <= 0.1: the second-order term is covered with room
        dq = u[:, 4:8]
        proj = (np.abs(qh) * dq).sum(1)                                # |d|q|| <= sum |qhat_j| |dq_j|
        ab[:, 4:8] += (dq + np.abs(qh) * proj[:, None]) / nc[:, None] * (1.0 + 2.0 * proj[:, None] / nc[:, None])
        ab[:, 11] += proj
        with np.errstate(over="ignore"):                               # (an unbounded input gives an unbounded output: inf, which callers reject)
            ab[:, 8:11] += np.exp(s) * np.expm1(u[:, 8:11])            # exact: e^(s+u) - e^s
    return act, Cond(rel, ab)


def chain(raw12, grad_act12, round_sigmoid=True):
    """Gradient w.r.t. the raw row from the gradient w.r.t. the activated row (columns 0..10; column 11 has none), as torch autograd
    forms it in fp32:  g y (1 - y) with y the fp32-ROUNDED sigmoid (round_sigmoid=False: the float64 one, for the check against
    float64 autograd),  (g - qhat (qhat . g)) / |q|,  g exp(s).  Not defined here for |q| < 1e-12 (torch's clamp makes the
    derivative g / 1e-12 there, the kernels keep the projection): callers do not draw such rows."""
    raw = np.asarray(raw12, np.float64).reshape(-1, 12)
    g = np.asarray(grad_act12, np.float64).reshape(raw.shape[0], -1)
    n = raw.shape[0]
    out = np.zeros((n, 12)); rel = np.zeros((n, 12)); ab = np.zeros((n, 12))
    out[:, 0:3] = g[:, 0:3]
    x = raw[:, 3]
    y = _sigmoid64(x)
    if round_sigmoid:
        y = f32(y)
    d = y * (1.0 - y)
    out[:, 3] = g[:, 3] * d
    # y itself is an fp32 result with activate()'s tolerance (K_ACT EPS y + EPS |x| y (1 - y) + underflow); d(y (1 - y)) = (1 - 2 y) dy.
    # Near y = 1 this term IS the tolerance: 1 - y is a multiple of 2^-24 there, in torch as in any fp32 evaluation.
    rel[:, 3] = np.abs(g[:, 3]) * (d + np.abs(1.0 - 2.0 * y) * y)
    ab[:, 3] = np.abs(g[:, 3]) * np.abs(1.0 - 2.0 * y) * (EPS * np.abs(x) * y * (1.0 - y) + FLT_MIN_NORMAL) + DENORM_STEP
    q = raw[:, 4:8]
    nq = np.sqrt((q * q).sum(1))
    assert (nq >= NORMALIZE_EPS).all(), "chain() is not defined below normalize's clamp"
    qh = q / nq[:, None]
    gq = g[:, 4:8]
    dot = (qh * gq).sum(1)
    out[:, 4:8] = (gq - qh * dot[:, None]) / nq[:, None]
    # cancellation scale of the projection; the dot product's own rounding error is EPS x sum_j |qhat_j g_j| (not EPS x |qhat . g|)
    rel[:, 4:8] = (np.abs(gq) + np.abs(qh) * (np.abs(qh) * np.abs(gq)).sum(1)[:, None]) / nq[:, None]
    ab[:, 4:8] = DENORM_STEP
    e = np.exp(raw[:, 8:11])
    out[:, 8:11] = g[:, 8:11] * e
    rel[:, 8:11] = np.abs(g[:, 8:11]) * e
    ab[:, 8:11] = np.abs(g[:, 8:11]) * EPS * np.abs(raw[:, 8:11]) * e + DENORM_STEP      # activate()'s expf term
    return out, Cond(rel, ab)


def chain_operator_norms(raw12):
    """Per row, the operator norm of each block's Jacobian (positions, density, rotation, scale): what a per-row scalar uncertainty
    of the activated gradient (the oracle's noise and flip budget) is multiplied by on its way to the raw parameters."""
    raw = np.asarray(raw12, np.float64).reshape(-1, 12)
    y = f32(_sigmoid64(raw[:, 3]))
    nq = np.maximum(np.sqrt((raw[:, 4:8] ** 2).sum(1)), NORMALIZE_EPS)
    return np.stack([np.ones(raw.shape[0]), y * (1.0 - y), 1.0 / nq, np.exp(raw[:, 8:11]).max(1)], 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# real spherical harmonics, degree <= 3, as sums of monomials  coefficient x^a y^b z^c  (closed-form constants; the CPU test holds
# them against oracle/per_ray_torch.py's, which tests/test_cpu_reference_pins.py pins to the reference's)
# ---------------------------------------------------------------------------------------------------------------------------------
_PI = math.pi
_K0 = 0.5 * math.sqrt(1.0 / _PI)
_K1 = math.sqrt(3.0 / (4.0 * _PI))
_K2A, _K2B, _K2C = 0.5 * math.sqrt(15.0 / _PI), 0.25 * math.sqrt(5.0 / _PI), 0.25 * math.sqrt(15.0 / _PI)
_K3A, _K3B, _K3C = 0.25 * math.sqrt(35.0 / (2.0 * _PI)), 0.5 * math.sqrt(105.0 / _PI), 0.25 * math.sqrt(21.0 / (2.0 * _PI))
_K3D, _K3E = 0.25 * math.sqrt(7.0 / _PI), 0.25 * math.sqrt(105.0 / _PI)
SH_MONOMIALS = (
    ((_K0, 0, 0, 0),),
    ((-_K1, 0, 1, 0),), ((_K1, 0, 0, 1),), ((-_K1, 1, 0, 0),),
    ((_K2A, 1, 1, 0),), ((-_K2A, 0, 1, 1),), ((2 * _K2B, 0, 0, 2), (-_K2B, 2, 0, 0), (-_K2B, 0, 2, 0)), ((-_K2A, 1, 0, 1),),
    ((_K2C, 2, 0, 0), (-_K2C, 0, 2, 0)),
    ((-3 * _K3A, 2, 1, 0), (_K3A, 0, 3, 0)), ((_K3B, 1, 1, 1),),
    ((-4 * _K3C, 0, 1, 2), (_K3C, 2, 1, 0), (_K3C, 0, 3, 0)),
    ((2 * _K3D, 0, 0, 3), (-3 * _K3D, 2, 0, 1), (-3 * _K3D, 0, 2, 1)),
    ((-4 * _K3C, 1, 0, 2), (_K3C, 3, 0, 0), (_K3C, 1, 2, 0)),
    ((_K3E, 2, 0, 1), (-_K3E, 0, 2, 1)), ((-_K3A, 3, 0, 0), (3 * _K3A, 1, 2, 0)),
)


def sh_basis(degree, d):
    """d [..,3] unit directions -> (Y [..,16], Yabs [..,16]); Y_k = 0 for k >= (degree+1)^2.  Yabs is the same sum with every
    monomial's absolute value: the condition scale of Y_k (2 zz - xx - yy cancels on a cone; its rounding error does not)."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = np.zeros(d.shape[:-1] + (16,)); A = np.zeros_like(Y)
    for k in range((degree + 1) ** 2):
        for c, a, b, e in SH_MONOMIALS[k]:
            t = c * x ** a * y ** b * z ** e
            Y[..., k] += t
            A[..., k] += np.abs(t)
    return Y, A


def sh_n_ops(degree):
    """Roundings an fp32 evaluation of a degree-`degree` basis function of normalize(pos - cam) carries, counted generously: the
    direction (one subtraction, three squares, two sums, a square root, a reciprocal, a product: 9, each entering `degree` times),
    the monomials (degree products) and their sum with the constants (3)."""
    return 10 * degree + 3


def sh_gradient(pos, cams, mrgb, degree, grad_scale):
    """pos [N,3], cams [V,3], mrgb [V,N,3] -> (G [N,48], unc [N,48]):  G[i, 3 k + c] = grad_scale sum_v Y_k(normalize(pos_i - cam_v))
    mrgb[v,i,c], columns beyond 3 (degree+1)^2 zero.  unc = sum_v Yabs_k |mrgb_v| grad_scale (n_ops(degree) + 2 + (V - 1)) EPS: the
    absolute uncertainty an fp32 evaluation of this gradient carries (the + 2: the products with grad_scale and with mrgb; V - 1: the
    running sum over the views rounds once per view added, each time relative to at most the sum of the absolute terms)."""
    pos = np.asarray(pos, np.float64); cams = np.asarray(cams, np.float64).reshape(-1, 3); mrgb = np.asarray(mrgb, np.float64)
    n = pos.shape[0]
    G = np.zeros((n, 16, 3)); U = np.zeros((n, 16, 3))
    gs = float(np.float32(grad_scale))
    for v in range(cams.shape[0]):
        d = pos - cams[v]
        dist = np.sqrt((d * d).sum(1))
        assert (dist > 0).all(), "a Gaussian exactly at a camera position has no direction: not drawn"
        Y, A = sh_basis(degree, d / dist[:, None])
        G += Y[:, :, None] * (mrgb[v] * gs)[:, None, :]
        U += A[:, :, None] * np.abs(mrgb[v] * gs)[:, None, :]
    return G.reshape(n, 48), (U * (sh_n_ops(degree) + 2 + (cams.shape[0] - 1)) * EPS).reshape(n, 48)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, lr_per_col, beta1, beta2, eps, step, visibility=None, g_unc=None):
    """One Adam step on [N,C] tensors, float64.  step >= 1: torch.optim.Adam's bias correction; step == 0: none (the reference's
    SelectiveAdam).  visibility [N] (optional): rows with 0 keep parameters AND moments.  g_unc: absolute uncertainty of g.
    Returns (p', m', v'), (Cond p, Cond m, Cond v)."""
    p = np.asarray(p, np.float64); g = np.asarray(g, np.float64); m = np.asarray(m, np.float64); v = np.asarray(v, np.float64)
    lr = f32(np.broadcast_to(np.asarray(lr_per_col, np.float64), (p.shape[1],)))[None, :]
    b1, b2, eps = float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(eps))
    bias1 = 1.0 - b1 ** step if step else 1.0
    bias2 = 1.0 - b2 ** step if step else 1.0
    dg = np.zeros_like(g) if g_unc is None else np.asarray(g_unc, np.float64)
    t1, t2 = b1 * m, (1.0 - b1) * g
    m2 = t1 + t2
    s_m = np.abs(t1) + np.abs(t2)
    v2 = b2 * v + (1.0 - b2) * g * g
    s_v = v2
    rb2 = math.sqrt(bias2)
    D = np.sqrt(v2) / rb2 + eps
    step_size = lr / bias1
    upd = step_size * m2 / D
    p2 = p - upd
    s_p = step_size * s_m / D
    # what v' may be off by besides its relative rounding: the gradient's own uncertainty, and three roundings (g g, its product with
    # 1 - beta2, the sum) that land in the denormal range when g^2 does
    dv = (1.0 - b2) * (2.0 * np.abs(g) * dg + dg * dg) + 3.0 * DENORM_STEP
    with np.errstate(divide="ignore", invalid="ignore"):
        dD = np.minimum(np.where(v2 > 0, dv / (2.0 * np.sqrt(v2)), np.inf), np.sqrt(dv)) / rb2   # |sqrt(a) - sqrt(b)| <= both
    ab_p = step_size * (1.0 - b1) * dg / D + np.abs(upd) * dD / np.maximum(D - dD, 0.5 * D)
    cp = Cond(s_p, ab_p)
    cp.abs += 0.5 * ulp32_up(np.abs(p2) + cp.abs + 64 * EPS * s_p)
    cm = Cond(s_m, (1.0 - b1) * dg + 2.0 * DENORM_STEP)      # (its two products may land in the denormal range)
    cm.abs += 0.5 * ulp32_up(np.abs(m2) + cm.abs + 64 * EPS * s_m)
    cv = Cond(s_v, dv)
    cv.abs += 0.5 * ulp32_up(np.abs(v2) + cv.abs + 64 * EPS * s_v)
    if visibility is not None:
        keep = ~(np.asarray(visibility).reshape(-1) != 0)
        for new, old, c in ((p2, p, cp), (m2, m, cm), (v2, v, cv)):
            new[keep] = old[keep]
            c.rel[keep] = 0.0; c.abs[keep] = 0.0       # untouched rows are compared bit for bit
    return (p2, m2, v2), (cp, cm, cv)


# ---------------------------------------------------------------------------------------------------------------------------------
# the MCMC regularisers (gut_hip.h: dL/dd = density_coeff sigmoid(d) (1 - sigmoid(d)), dL/ds_k = scale_coeff exp(s_k))
# ---------------------------------------------------------------------------------------------------------------------------------
def regulariser(raw12, density_coeff, scale_coeff):
    """-> (g12 [N,12] with the two gradient terms in columns 3 and 8..10, Cond, partials [ceil(N/64),2] = per 64-row wave (sum of
    sigmoid, sum of exp(s_k)) )."""
    raw = np.asarray(raw12, np.float64).reshape(-1, 12)
    n = raw.shape[0]
    coeff = np.zeros((n, 12))
    coeff[:, 3] = float(np.float32(density_coeff))
    coeff[:, 8:11] = float(np.float32(scale_coeff))
    g, c = chain(np.where(np.arange(12)[None, :] == 7, 1.0, raw), coeff)   # (column 7 := 1: the unused rotation block stays defined)
    g[:, 0:3] = 0.0; g[:, 4:8] = 0.0
    c.rel[:, 0:3] = 0.0; c.rel[:, 4:8] = 0.0; c.abs[:, 0:3] = 0.0; c.abs[:, 4:8] = 0.0
    waves = (n + 63) // 64
    pad = np.zeros((waves * 64, 2))
    pad[:n, 0] = _sigmoid64(raw[:, 3])
    pad[:n, 1] = np.exp(raw[:, 8:11]).sum(1)
    return g, c, pad.reshape(waves, 64, 2).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# one fused step (gut_sh_adam_step*): Adam on the raw row, then on the [N,48] row with the SH gradient rebuilt from the PRE-update
# position; both gradients scaled by grad_scale, the regulariser added after that scaling; the new activated row
# ---------------------------------------------------------------------------------------------------------------------------------
def step(raw12, m12, v12, sh48, m48, v48, grad12, cams, mrgb, degree, grad_scale, lr12, lr48, beta1, beta2, eps, step_no,
         visibility=None, reg=None, g12_unc=None, g48=None, g48_unc=None):
    """Returns dict(raw12, m12, v12, sh48, m48, v48, act12) -> (value float64, Cond).  grad12 [N,12]: gradient w.r.t. the raw row
    (column 11, the unused one, takes a zero gradient).  reg = (density_coeff, scale_coeff) or None.  g48 / g48_unc: a ready [N,48]
    gradient and its uncertainty instead of (cams, mrgb).  Rows with visibility 0: everything untouched, act12 included (its Cond is
    zero there and its value is NaN: the caller compares those rows with what it had)."""
    raw = np.asarray(raw12, np.float64).reshape(-1, 12)
    gs = float(np.float32(grad_scale))
    g = np.asarray(grad12, np.float64).reshape(-1, 12) * gs
    g[:, 11] = 0.0
    gu = np.abs(g) * EPS if g12_unc is None else np.asarray(g12_unc, np.float64) * gs + np.abs(g) * EPS   # the product with grad_scale rounds
    if reg is not None:
        rg, rc, _ = regulariser(raw, reg[0], reg[1])
        g = g + rg
        gu = gu + rc.bound(K_CHAIN) + np.abs(g) * EPS
    (p, m, v), (cp, cm, cv) = adam(raw, g, m12, v12, lr12, beta1, beta2, eps, step_no, visibility, gu)
    if g48 is None:
        g48, g48_unc = sh_gradient(raw[:, 0:3], cams, mrgb, degree, grad_scale)
    (s, sm, sv), (cs, csm, csv) = adam(sh48, g48, m48, v48, lr48, beta1, beta2, eps, step_no, visibility, g48_unc)
    act, ca = activate(p, raw_unc=cp.bound(K_ADAM))
    ca = Cond(np.zeros_like(act), ca.bound(K_ACT))      # both constants are in: the bound is final
    if visibility is not None:
        keep = ~(np.asarray(visibility).reshape(-1) != 0)
        act[keep] = np.nan
        ca.abs[keep] = 0.0
    return dict(raw12=(p, cp), m12=(m, cm), v12=(v, cv), sh48=(s, cs), m48=(sm, csm), v48=(sv, csv), act12=(act, ca))


# ---------------------------------------------------------------------------------------------------------------------------------
# the input table of the element tests (seeded): what a block L2 on a random scene never reaches
# ---------------------------------------------------------------------------------------------------------------------------------
def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), shape))


def draw_adam_inputs(n, cols, seed, beta1=0.9, zero_rows=True):
    """-> p, g, m, v  [n, cols] float32.  v log-uniform 1e-44..1e+20 with 5 % zeros and dense bands around 2^-96 and 2^-126;
    m = +-sqrt(v) U(0,3) with zeros and with beta1 m cancelling (1 - beta1) g to 1e-3; g = +-log-uniform 1e-22..1e+8, 10 % zero
    elements, 30 % zero rows; p = +-log-uniform 1e-6..1e+3, 5 % zeros."""
    rng = np.random.default_rng(seed)
    sh = (n, cols)
    v = _log_uniform(rng, 1e-44, 1e20, sh)
    band = rng.random(sh)
    v = np.where(band < 0.10, 2.0 ** -96 * np.exp(rng.uniform(-0.7, 0.7, sh)), v)
    v = np.where((band >= 0.10) & (band < 0.18), 2.0 ** -126 * np.exp(rng.uniform(-2.0, 2.0, sh)), v)
    v = np.where((band >= 0.18) & (band < 0.23), 0.0, v)
    v = v.astype(np.float32)
    g = (rng.choice([-1.0, 1.0], sh) * _log_uniform(rng, 1e-22, 1e8, sh))
    g = np.where(rng.random(sh) < 0.10, 0.0, g)
    if zero_rows:
        g = np.where(rng.random((n, 1)) < 0.30, 0.0, g)
    g = g.astype(np.float32)
    m = rng.choice([-1.0, 1.0], sh) * np.sqrt(v.astype(np.float64)) * rng.uniform(0.0, 3.0, sh)
    m = np.where(rng.random(sh) < 0.05, 0.0, m)
    b1 = float(np.float32(beta1))
    cancel = rng.random(sh) < 0.10
    m = np.where(cancel, -(1.0 - b1) * g.astype(np.float64) / b1 * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, sh)), m)
    m = m.astype(np.float32)
    # |m| <= 3 sqrt(v) everywhere, the cancelling draws included (a first moment cannot exceed the root of the second by more in
    # any Adam history, and without it a zero-gradient step moves a parameter by 1e17)
    v = np.where(cancel, np.maximum(v.astype(np.float64), (m.astype(np.float64) / 3.0) ** 2 * (1.0 + 1e-6)), v).astype(np.float32)
    p = rng.choice([-1.0, 1.0], sh) * _log_uniform(rng, 1e-6, 1e3, sh)
    p = np.where(rng.random(sh) < 0.05, 0.0, p).astype(np.float32)
    return p, g, m, v


EXTREME_LOGITS = (-100.0, -88.8, -87.0, -30.0, -17.0, 0.0, 17.0, 30.0, 89.0)
QUAT_NORMS = (1e-20, float(np.nextafter(np.float32(1e-12), np.float32(0))), float(np.float32(1e-12)),
              float(np.nextafter(np.float32(1e-12), np.float32(1))), 1e-6, 1.0, 1e6)


def draw_raw_rows(n, seed, clamp_free=False, cameras=None):
    """Raw rows [n,12] float32 at the edges of the activations: logits including EXTREME_LOGITS, log-scales -20..+10, quaternions of
    the norms QUAT_NORMS and (0,0,0,0).  clamp_free: no quaternion below normalize's clamp (for chain()).  cameras [V,3]: rows 0 / 1
    (when present) are placed 1e-3 / 1e+4 from camera 0; no row sits exactly on a camera."""
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, 12))
    raw[:, 0:3] = rng.choice([-1.0, 1.0], (n, 3)) * _log_uniform(rng, 1e-3, 30.0, (n, 3))
    raw[:, 3] = rng.uniform(-20.0, 20.0, n)
    k = rng.integers(0, 3 * len(EXTREME_LOGITS), n)
    raw[:, 3] = np.where(k < len(EXTREME_LOGITS), np.asarray(EXTREME_LOGITS)[k % len(EXTREME_LOGITS)], raw[:, 3])
    q = rng.normal(size=(n, 4))
    q /= np.sqrt((q * q).sum(1, keepdims=True))
    norms = np.asarray(QUAT_NORMS[4:] if clamp_free else QUAT_NORMS)
    pick = rng.integers(0, len(norms) + 2, n)
    scale = np.where(pick < len(norms), norms[pick % len(norms)], 10.0 ** rng.uniform(-3.0, 3.0, n))
    raw[:, 4:8] = q * scale[:, None]
    if not clamp_free:
        raw[rng.random(n) < 0.03, 4:8] = 0.0
    raw[:, 8:11] = rng.uniform(-20.0, 10.0, (n, 3))
    raw[:, 11] = rng.normal(size=n)
    if cameras is not None:
        c0 = np.asarray(cameras, np.float64).reshape(-1, 3)[0]
        u = np.array([0.6, -0.48, 0.64])
        if n > 0:
            raw[0, 0:3] = c0 + 1e-3 * u
        if n > 1:
            raw[1, 0:3] = c0 + 1e4 * u
    return raw.astype(np.float32)


def lr_ladder(cols, lo=1e-5, hi=5e-2):
    """All columns different: a geometric ladder, so that a column mix-up moves a result."""
    return np.geomspace(lo, hi, cols).astype(np.float32)


STEPS = (0, 1, 2, 10, 1000, 1023, 1024, 1025, 30000, 10 ** 6)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4097, 100003)
