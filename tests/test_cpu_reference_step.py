"""tests/reference_step.py against things the project did not write (torch in float64, the closed form of the reference's
SelectiveAdam, the oracle's SH basis), and the MEASUREMENT of its tolerance constants: two legitimate float32 evaluations of every
operation against float64 on the whole input table, bounded on every element by the model with K / K_BAND (tests/common.py)."""
import importlib
import itertools

import numpy as np
import pytest
import torch

from tests import reference_step as R
from tests.common import K_ACT, K_ADAM, K_ADAM_IEEE, K_BAND, K_CHAIN, K_MOMENT

EPS = R.EPS
B1, B2 = 0.9, 0.999


# ---- the restatement against torch float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 10])
def test_adam_is_torch_optim_adam_in_float64(steps):
    rng = np.random.default_rng(steps)
    n, cols = 37, 12
    lr = R.lr_ladder(cols)
    b1, b2, eps = float(np.float32(B1)), float(np.float32(B2)), float(np.float32(1e-15))
    p0 = rng.normal(size=(n, cols)).astype(np.float32)
    params = [torch.nn.Parameter(torch.tensor(p0[:, i:i + 1], dtype=torch.float64)) for i in range(cols)]
    opt = torch.optim.Adam([dict(params=[c], lr=float(lr[i])) for i, c in enumerate(params)], betas=(b1, b2), eps=eps)
    p, m, v = p0.astype(np.float64), np.zeros((n, cols)), np.zeros((n, cols))
    for t in range(1, steps + 1):
        g = (rng.normal(size=(n, cols)) * 10.0 ** rng.uniform(-6, 2, (n, cols))).astype(np.float32)
        for i, c in enumerate(params):
            c.grad = torch.tensor(g[:, i:i + 1], dtype=torch.float64)
        opt.step()
        (p, m, v), _ = R.adam(p, g, m, v, lr, B1, B2, 1e-15, t)
    ref = torch.cat([c.detach() for c in params], 1).numpy()
    assert np.abs(p - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    st = opt.state[params[3]]
    assert np.allclose(m[:, 3:4], st["exp_avg"].numpy(), rtol=1e-12, atol=0) and np.allclose(v[:, 3:4], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_selective_adam_closed_form_and_untouched_rows():
    """optimizers.cu:47-79: m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g g, p += -lr m' / (sqrt(v') + eps), invisible rows untouched."""
    p, g, m, v = R.draw_adam_inputs(257, 4, 7)
    vis = (np.arange(257) % 3 != 0)
    (p2, m2, v2), (cp, cm, cv) = R.adam(p, g, m, v, np.full(4, 0.01, np.float32), B1, B2, 1e-8, 0, visibility=vis)
    b1, b2, eps, lr = (float(np.float32(x)) for x in (B1, B2, 1e-8, 0.01))
    P, G, M, V = (a.astype(np.float64) for a in (p, g, m, v))
    em = b1 * M + (1 - b1) * G; ev = b2 * V + (1 - b2) * G * G
    ep = P + -lr * em / (np.sqrt(ev) + eps)
    assert np.array_equal(p2[vis], ep[vis]) or np.allclose(p2[vis], ep[vis], rtol=1e-14, atol=0)
    assert np.allclose(m2[vis], em[vis], rtol=1e-15, atol=0) and np.allclose(v2[vis], ev[vis], rtol=1e-15, atol=0)
    assert np.array_equal(p2[~vis], P[~vis]) and np.array_equal(m2[~vis], M[~vis]) and np.array_equal(v2[~vis], V[~vis])
    assert not cp.bound(K_ADAM)[~vis].any() and not cm.bound(K_ADAM)[~vis].any() and not cv.bound(K_ADAM)[~vis].any()


def test_activate_and_chain_are_torch_autograd_in_float64():
    raw = R.draw_raw_rows(4000, 11, clamp_free=True)
    rng = np.random.default_rng(5)
    gact = (rng.normal(size=(4000, 12)) * 10.0 ** rng.uniform(-8, 4, (4000, 12))).astype(np.float32)
    t = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    act = torch.cat([t[:, 0:3], torch.sigmoid(t[:, 3:4]), torch.nn.functional.normalize(t[:, 4:8], dim=1), torch.exp(t[:, 8:11])], 1)
    a64, _ = R.activate(raw)
    assert np.allclose(a64[:, :11], act.detach().numpy(), rtol=1e-13, atol=1e-300)
    assert np.allclose(a64[:, 11], t[:, 4:8].detach().norm(dim=1).clamp_min(1e-12).numpy(), rtol=1e-14)
    act.backward(torch.tensor(gact[:, :11], dtype=torch.float64))
    got, cond = R.chain(raw, gact, round_sigmoid=False)
    want = t.grad.numpy()
    # float64 against float64: 1e-12 of the condition scale
    assert (np.abs(got[:, :11] - want[:, :11]) <= 1e-12 * cond.rel[:, :11] + 1e-300).all()
    assert not got[:, 11].any()
    # the fp32-rounded sigmoid of the default form differs from the exact derivative by tens of per cent at logit 17 — torch's own fp32 behaviour
    r17 = raw.copy(); r17[:, 3] = 17.0
    a, _ = R.chain(r17, gact); b, _ = R.chain(r17, gact, round_sigmoid=False)
    nz = gact[:, 3] != 0
    assert 0.2 < np.abs(a[nz, 3] / b[nz, 3] - 1).max() < 0.6
    norms = R.chain_operator_norms(raw)
    chained = R.chain(raw, gact)[0]
    for j, sl in enumerate((slice(0, 3), slice(3, 4), slice(4, 8), slice(8, 11))):
        assert (np.linalg.norm(chained[:, sl], axis=1) <= np.linalg.norm(gact[:, sl].astype(np.float64), axis=1) * norms[:, j] * (1 + 1e-9)).all()


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_basis_and_gradient_against_the_oracles(degree):
    prt = importlib.import_module("oracle.per_ray_torch")
    rng = np.random.default_rng(degree)
    d = rng.normal(size=(500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, A = R.sh_basis(degree, d)
    want = prt.sh_basis(degree, torch.tensor(d)).numpy()
    nc = (degree + 1) ** 2
    assert np.abs(Y[:, :nc] - want).max() <= 1e-14 and not Y[:, nc:].any() and (A >= np.abs(Y) - 1e-15).all()
    # the [N,48] gradient = d/d(sph48) of sum_v <mrgb_v, colour_v>, colour from the oracle's precompute_features, by float64 autograd
    pos = rng.normal(size=(500, 3)).astype(np.float32); cams = (rng.normal(size=(3, 3)) * 4).astype(np.float32)
    mrgb = rng.normal(size=(3, 500, 3)).astype(np.float32)
    sph = torch.zeros((500, 48), dtype=torch.float64, requires_grad=True)
    loss = sum((prt.precompute_features(torch.tensor(pos, dtype=torch.float64), sph, torch.tensor(cams[v], dtype=torch.float64), degree)
                * torch.tensor(mrgb[v], dtype=torch.float64)).sum() for v in range(3))
    (0.5 * loss).backward()
    G, U = R.sh_gradient(pos, cams, mrgb, degree, 0.5)
    assert np.abs(G - sph.grad.numpy()).max() <= 1e-13 and not G[:, 3 * nc:].any() and not U[:, 3 * nc:].any()


def test_regulariser_is_the_gradient_of_the_documented_losses():
    raw = R.draw_raw_rows(1000, 3)
    raw[:, 3] = np.clip(raw[:, 3], -30, 12)        # (float64 autograd of the exact sigmoid; the fp32-rounded y is compared below 12)
    n = raw.shape[0]
    lam_o, lam_s = 0.01, 0.02
    t = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    (lam_o * torch.sigmoid(t[:, 3]).abs().mean() + lam_s * torch.exp(t[:, 8:11]).abs().mean()).backward()
    g, c, partials = R.regulariser(raw, lam_o / n, lam_s / (3 * n))
    assert (np.abs(g - t.grad.numpy()) <= c.bound(K_CHAIN)).all()
    assert partials.shape == ((n + 63) // 64, 2)
    assert np.isclose(partials[:, 0].sum(), torch.sigmoid(t[:, 3]).sum().item(), rtol=1e-12)
    assert np.isclose(partials[:, 1].sum(), torch.exp(t[:, 8:11]).sum().item(), rtol=1e-12)


def test_reference_is_finite_on_the_whole_input_table():
    for n in R.SIZES:
        p, g, m, v = R.draw_adam_inputs(n, 48, n)
        for t, eps in itertools.product(R.STEPS, (1e-15, 1e-8)):
            outs, conds = R.adam(p, g, m, v, R.lr_ladder(48), B1, B2, eps, t)
            assert all(np.isfinite(o).all() for o in outs) and all(np.isfinite(c.bound(K_ADAM)).all() for c in conds), (n, t, eps)
            if n > 1000:
                break
    cams = np.array([[0.5, -1.0, -4.0], [3.0, 0.2, 1.0]], np.float32)
    raw = R.draw_raw_rows(4097, 1, cameras=cams)
    a, c = R.activate(raw)
    assert np.isfinite(a).all() and np.isfinite(c.bound(K_ACT)).all()
    rng = np.random.default_rng(0)
    G, U = R.sh_gradient(raw[:, :3], cams, rng.normal(size=(2, 4097, 3)).astype(np.float32), 3, 0.5)
    assert np.isfinite(G).all() and np.isfinite(U).all()
    g, c, partials = R.regulariser(raw, 1e-6, 3e-7)
    assert np.isfinite(g).all() and np.isfinite(c.bound(K_CHAIN)).all() and np.isfinite(partials).all()


# ---- the measurement: two float32 evaluations against float64 -----------------------------------------------------------------
def _f(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    """a b + c rounded once (the product of two fp32 values is exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _shift(x, k):
    """x moved by k in {-1, 0, +1} ulp: the specified accuracy of the hardware reciprocal and square root."""
    up = np.nextafter(x, np.float32(np.inf)); dn = np.nextafter(x, np.float32(-np.inf))
    return np.where(k > 0, up, np.where(k < 0, dn, x)).astype(np.float32)


def _adam_ieee(p, g, m, v, lr, b1, b2, eps, step):
    """form (a): one rounding per operation, IEEE division and square root, bias corrections divided by on the device"""
    b1, b2, eps = np.float32(b1), np.float32(b2), np.float32(eps)
    bias1 = np.float32(1.0 - float(b1) ** step) if step else np.float32(1)
    bias2s = np.float32(np.sqrt(1.0 - float(b2) ** step)) if step else np.float32(1)
    one = np.float32(1)
    mm = b1 * m + (one - b1) * g
    vv = b2 * v + (one - b2) * g * g
    pp = p - (_f(lr)[None, :] / bias1) * mm / (np.sqrt(vv) / bias2s + eps)
    return pp, mm, vv


def _adam_ieee_fma(p, g, m, v, lr, b1, b2, eps, step):
    """form (a'): form (a) with the two moment sums and the final subtraction rounded once (FMA) — what contraction makes of the IEEE
    kernels' source; division and square root stay IEEE"""
    b1, b2, eps = np.float32(b1), np.float32(b2), np.float32(eps)
    bias1 = np.float32(1.0 - float(b1) ** step) if step else np.float32(1)
    bias2s = np.float32(np.sqrt(1.0 - float(b2) ** step)) if step else np.float32(1)
    one = np.float32(1)
    mm = _fma(np.broadcast_to(b1, m.shape), m, (one - b1) * g)
    vv = _fma(np.broadcast_to(b2, v.shape), v, ((one - b2) * g) * g)
    pp = p - (_f(lr)[None, :] / bias1) * mm / (np.sqrt(vv) / bias2s + eps)
    return pp, mm, vv


def _adam_fast(p, g, m, v, lr, b1, b2, eps, step, rng):
    """form (b): products rounded once (FMA), reciprocals of the bias corrections formed on the host, 1/x and sqrt(x) each within
    one ulp of the correctly rounded value"""
    b1, b2, eps = np.float32(b1), np.float32(b2), np.float32(eps)
    bias1 = np.float32(1.0 - float(b1) ** step) if step else np.float32(1)
    bias2s = np.float32(np.sqrt(1.0 - float(b2) ** step)) if step else np.float32(1)
    one = np.float32(1)
    lr_b = (_f(lr) / bias1)[None, :]
    inv_b2 = one / bias2s
    mm = _fma(np.broadcast_to(b1, m.shape), m, (one - b1) * g)
    vv = _fma(np.broadcast_to(b2, v.shape), v, ((one - b2) * g) * g)
    s = _shift(np.sqrt(vv), rng.integers(-1, 2, vv.shape))
    s = np.maximum(s, np.float32(0))
    d = _fma(s, np.broadcast_to(inv_b2, s.shape), np.broadcast_to(eps, s.shape))
    r = _shift(one / d, rng.integers(-1, 2, d.shape))
    pp = _fma(-(lr_b * mm), r, p)
    return pp, mm, vv


def test_two_float32_evaluations_measure_K_ADAM():
    """Asserts on EVERY element of the input table that |fp32 form - float64| <= (K / K_BAND) EPS S + the non-scaling terms and prints
    the worst ratio (tests/common.py records it).  K: K_ADAM for the parameter in the fast form (b), K_ADAM_IEEE for the parameter in
    the IEEE forms (a) and (a'), K_MOMENT for both moments in every form."""
    rng = np.random.default_rng(0)
    worst = {}
    with np.errstate(all="ignore"):
        for n, cols in ((4097, 12), (4097, 48), (1000, 4)):
            lr = R.lr_ladder(cols)
            for t, eps in itertools.product(R.STEPS, (1e-15, 1e-8)):
                p, g, m, v = R.draw_adam_inputs(n, cols, 1000 * t % 9973 + cols)
                outs, conds = R.adam(p, g, m, v, lr, B1, B2, eps, t)
                for form, got in (("ieee", _adam_ieee(p, g, m, v, lr, B1, B2, eps, t)), ("ieee_fma", _adam_ieee_fma(p, g, m, v, lr, B1, B2, eps, t)), ("fast", _adam_fast(p, g, m, v, lr, B1, B2, eps, t, rng))):
                    for name, o, c, x in zip("pmv", outs, conds, got):
                        err = np.abs(x.astype(np.float64) - o)
                        ratio = np.where(c.rel > 0, np.maximum(err - c.abs, 0) / np.maximum(EPS * c.rel, 1e-300), 0.0)
                        worst[(form, name)] = max(worst.get((form, name), 0.0), float(ratio.max()))
                        K = K_MOMENT if name in "mv" else (K_ADAM if form == "fast" else K_ADAM_IEEE)
                        bad = err > c.bound(K / K_BAND)
                        assert not bad.any(), (form, name, t, eps, int(bad.sum()), float(ratio.max()))
    print(f"[band K_ADAM] worst (err - abs terms) / (EPS S): {worst}; K / K_BAND = {K_ADAM / K_BAND} (fast p), {K_ADAM_IEEE / K_BAND} (IEEE p), {K_MOMENT / K_BAND} (m, v)")


def _activate32_numpy(raw):
    raw = _f(raw); one = np.float32(1)
    with np.errstate(all="ignore"):
        y = one / (one + np.exp(-raw[:, 3]))
        q = raw[:, 4:8]
        nrm = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        nc = np.maximum(nrm, np.float32(1e-12))
        return np.concatenate([raw[:, 0:3], y[:, None], q * (one / nc)[:, None], np.exp(raw[:, 8:11]), nc[:, None]], 1)


def _activate32_torch(raw):
    t = torch.tensor(raw)
    return torch.cat([t[:, 0:3], torch.sigmoid(t[:, 3:4]), torch.nn.functional.normalize(t[:, 4:8], dim=1), torch.exp(t[:, 8:11]),
                      t[:, 4:8].norm(dim=1, keepdim=True).clamp_min(1e-12)], 1).numpy()


def test_two_float32_evaluations_measure_K_ACT():
    worst = {}
    raw = R.draw_raw_rows(100003, 2)
    a64, c = R.activate(raw)
    for form, got in (("numpy", _activate32_numpy(raw)), ("torch", _activate32_torch(raw))):
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - a64)
        ratio = np.where(c.rel > 0, np.maximum(err - c.abs, 0) / np.maximum(EPS * c.rel, 1e-300), 0.0)
        worst[("activate", form)] = float(ratio.max())
        assert (err <= c.bound(K_ACT / K_BAND)).all(), (form, float(ratio.max()), np.argwhere(err > c.bound(K_ACT / K_BAND))[:5])
    # chain: torch autograd in float32 through its own float32 activations, and the same formulas in numpy float32
    raw = R.draw_raw_rows(100003, 3, clamp_free=True)
    rng = np.random.default_rng(4)
    gact = (rng.normal(size=(raw.shape[0], 12)) * 10.0 ** rng.uniform(-8, 4, (raw.shape[0], 12))).astype(np.float32)
    gact[:, 11] = 0
    want, c = R.chain(raw, gact)
    t = torch.tensor(raw, requires_grad=True)
    act = torch.cat([t[:, 0:3], torch.sigmoid(t[:, 3:4]), torch.nn.functional.normalize(t[:, 4:8], dim=1), torch.exp(t[:, 8:11])], 1)
    act.backward(torch.tensor(gact[:, :11]))
    a32 = _activate32_numpy(raw)
    with np.errstate(all="ignore"):
        one = np.float32(1)
        dot = (gact[:, 4:8] * a32[:, 4:8]).sum(1, dtype=np.float32)
        np32 = np.concatenate([gact[:, 0:3], (gact[:, 3] * a32[:, 3] * (one - a32[:, 3]))[:, None],
                               (gact[:, 4:8] - a32[:, 4:8] * dot[:, None]) * (one / a32[:, 11])[:, None], gact[:, 8:11] * a32[:, 8:11],
                               np.zeros((raw.shape[0], 1), np.float32)], 1)
    for form, got in (("torch", np.concatenate([t.grad.numpy()[:, :11], np.zeros((raw.shape[0], 1), np.float32)], 1)), ("numpy", np32)):
        err = np.abs(got.astype(np.float64) - want)
        ratio = np.where(c.rel > 0, np.maximum(err - c.abs, 0) / np.maximum(EPS * c.rel, 1e-300), 0.0)
        worst[("chain", form)] = float(ratio.max())
        assert (err <= c.bound(K_CHAIN / K_BAND)).all(), (form, float(ratio.max()), np.argwhere(err > c.bound(K_CHAIN / K_BAND))[:5])
    print(f"[band K_ACT, K_CHAIN] worst (err - abs terms) / (EPS scale): {worst}; K_ACT / K_BAND = {K_ACT / K_BAND}, K_CHAIN / K_BAND = {K_CHAIN / K_BAND}")


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_float32_sh_gradient_stays_inside_its_uncertainty(degree):
    """sh_gradient's `unc` is a count of roundings, not a measured constant: a float32 evaluation (direction by one reciprocal square
    root, monomials and sums rounded one by one) must stay inside unc / K_BAND on every element, including a Gaussian 1e-3 and 1e+4
    from a camera and directions on the cones where a basis function cancels."""
    rng = np.random.default_rng(degree)
    cams = np.array([[0.5, -1.0, -4.0], [3.0, 0.2, 1.0], [-2.0, 2.5, 0.3], [0.0, 0.0, 9.0], [1.0, 1.0, 1.0]], np.float32)
    raw = R.draw_raw_rows(20000, degree, cameras=cams)
    pos = raw[:, :3].copy()
    # directions on 2 zz = xx + yy seen from camera 2
    k = np.arange(100, 600)
    ph = rng.uniform(0, 2 * np.pi, k.size)
    pos[k] = cams[2] + (rng.uniform(0.5, 5, k.size)[:, None] * np.stack([np.cos(ph), np.sin(ph), np.full(k.size, np.sqrt(0.5))], 1)).astype(np.float32)
    mrgb = (rng.normal(size=(5, pos.shape[0], 3)) * 10.0 ** rng.uniform(-6, 2, (5, pos.shape[0], 1))).astype(np.float32)
    G, U = R.sh_gradient(pos, cams, mrgb, degree, 0.2)
    gs = np.float32(0.2)
    acc = np.zeros((pos.shape[0], 16, 3), np.float32)
    for v in range(5):
        d = pos - cams[v]
        inv = np.float32(1) / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        d = d * inv[:, None]
        Y = np.zeros((pos.shape[0], 16), np.float32)
        for kk in range((degree + 1) ** 2):
            for cf, a, b, e in R.SH_MONOMIALS[kk]:
                term = np.full(pos.shape[0], np.float32(cf))
                for comp, power in ((0, a), (1, b), (2, e)):
                    for _ in range(power):
                        term = term * d[:, comp]
                Y[:, kk] += term
        acc += Y[:, :, None] * (mrgb[v] * gs)[:, None, :]
    err = np.abs(acc.reshape(-1, 48).astype(np.float64) - G)
    ratio = float((err / np.maximum(U, 1e-300)).max())
    print(f"[band SH degree {degree}] worst |fp32 - fp64| / unc = {ratio:.3f}")
    assert (err <= U / K_BAND + R.DENORM_STEP).all(), ratio
