"""The oracle's per-hit arithmetic against the reference's OWN code.

tests/golden/hit_golden.npz records what the reference's per-hit header (kernels/cuda/models/gaussianParticles.cuh with
common/mathUtils.cuh under it), compiled for the host behind oracle/ref_host/shim.h, returned for seeded inputs
(tests/golden/gen_hit_golden.py).  Variant 0 of oracle/gut_oracle.c is DEFINED as "the reference's operation order, no contraction,
libm": here that sentence is checked, bit for bit, unit by unit — response and response gradient of the seven kernels, one
processHitBwd<n, false, false> step (accept decision, updated running state, 11-float density gradient, 3-float feature gradient), SH
radiance and its backward, quaternion to rows — through exported wrappers of the very static functions render_bwd_impl,
oracle_project and oracle_project_bwd use.  Then oracle.backward on one composed 48 x 40 scene per degree against per-Gaussian sums of
the reference's per-hit gradients walked over the same tile lists.

No output needed an exception: every one is bit-equal (NaN compares equal to NaN of the same bit pattern; the linear kernel's
gradient at squared distance 0 is 0 x inf in the reference, and in the oracle).

Not covered, because the reference's code for it cannot be built without nvcc / slangc / tiny-cuda-nn: the forward's per-hit function
(Slang), the camera projection and tile tests, the renderer's loops.  The branch `galpha >= 0.999999` of processHitBwd
(gaussianParticles.cuh:573) is unreachable under `galpha = fminf(0.99f, .)` (:528) and is left to reading.
"""
import importlib

import numpy as np
import pytest

from tests import reference_hit_cases as rc
from tests.common import cams, make_view

oracle = importlib.import_module("oracle.oracle")

# oracle.backward against the recorded sums on scene (c).  The per-hit terms are bit-equal and both sides sum them in double, so the
# [12,12] rows differ by the rounding of double sums of ~1e3..1e4 terms taken in another order (OpenMP atomics): MEASURED worst
# |difference| / |row| over the seven degrees, 39 runs at 1 to 64 threads, 2.0e-16.  The [12,48] rows go through the reference's fp32 radianceFromSpHBwd (the
# summed feature gradient rounded to fp32, fp32 products) on the fixture's side and through double products on the oracle's: MEASURED
# 6.3e-8 (the fp32 roundings of the cotangent and of the product, 2^-24 = 6.0e-8 each).  Asserted: ten times the measured values.
SCENE_G12_MEASURED, SCENE_G48_MEASURED = 2.0e-16, 6.3e-8


@pytest.fixture(scope="module")
def golden():
    with np.load(rc.GOLDEN) as z:
        assert all(z[k].dtype.kind in "fiu" for k in z.files), "the fixture holds numeric arrays only"
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def units():
    assert oracle.lib().oracle_get_variant() == 0
    return oracle.HitUnits()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero((bits(got) != bits(want)).reshape(got.shape[0], -1).any(1))[0] if got.ndim else np.nonzero(bits(got) != bits(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0] if got.ndim else 1} cases differ, first {bad[:8]}: got {got[bad[0]]}, reference {want[bad[0]]}"


def run_hit_cases(u, degree, g):
    n = rc.CASES_PER_DEGREE
    out = dict(accepted=np.zeros(n, np.int32), state_after=np.zeros((n, 5), np.float32), density_grad=np.zeros((n, 11), np.float32),
               feat_grad=np.zeros((n, 3), np.float32))
    k = lambda name: g[f"hit{degree}_{name}"]
    for i in range(n):
        a, st, g11, g3 = u.hit_bwd(degree, k("ray_ori")[i], k("ray_dir")[i], k("particle")[i], k("feat")[i], g["thresholds"], k("finals")[i],
                                   k("cot")[i], k("state")[i])
        out["accepted"][i] = a; out["state_after"][i] = st; out["density_grad"][i] = g11; out["feat_grad"][i] = g3
    return out


def run_responses(u, degree, g):
    resp = np.array([u.response(degree, v) for v in g["resp_d2"]], np.float32)
    grad = np.array([u.response_grad(degree, a, b, c) for a, b, c in zip(g["resp_d2"], g[f"resp{degree}"], g["resp_cot"])], np.float32)
    return resp, grad


def run_sh(u, deg, g):
    cl = np.stack([u.sh_radiance(deg, r, d, True) for r, d in zip(g["sh_rows"], g["sh_dir"])])
    un = np.stack([u.sh_radiance(deg, r, d, False) for r, d in zip(g["sh_rows"], g["sh_dir"])])
    gr = np.stack([u.sh_radiance_bwd(deg, d, c, x) for d, c, x in zip(g["sh_dir"], g["sh_cot"], g[f"sh{deg}_unclamped"])])
    return cl, un, gr


def test_fixture_holds_the_cases_the_units_can_go_wrong_on(golden):
    assert tuple(golden["degrees"]) == rc.DEGREES and np.array_equal(golden["thresholds"], rc.THRESHOLDS)
    for n in rc.DEGREES:
        k = lambda name: golden[f"hit{n}_{name}"]
        assert k("ray_ori").shape == (rc.CASES_PER_DEGREE, 3)
        pop = rc.check_populations(n, rc.hit_classes(n, k("ray_ori"), k("ray_dir"), k("particle"), k("feat"), k("finals"), k("state"), k("accepted")))
        print(f"[hit classes, degree {n}] {pop}")
        rej = k("accepted") == 0       # a rejected hit leaves the state alone and writes no gradient
        assert_bit_equal(k("state_after")[rej], k("state")[rej], "state of rejected hits")
        assert not k("density_grad")[rej].any() and not k("feat_grad")[rej].any()
        assert np.nan_to_num(np.abs(k("density_grad")[~rej]), nan=1.0).max(1).min() > 0     # (NaN: the linear kernel at distance 0)
    assert golden["sh_dir"].shape == (rc.SH_CASES, 3) and golden["sh_rows"].shape == (rc.SH_CASES, 48)
    for deg in range(4):
        un = golden[f"sh{deg}_unclamped"]
        assert int((un <= 0).any(1).sum()) >= rc.MIN_CLASS and int((un > 0).all(1).sum()) >= rc.MIN_CLASS
        assert not golden[f"sh{deg}_grad"].reshape(-1, 16, 3)[:, (deg + 1) ** 2:].any()
    assert golden["scene_d12"].shape == (12, 12) and golden["scene_rgba_grad"].shape == (rc.SCENE_H, rc.SCENE_W, 4)
    assert all(np.abs(golden[k]).min() > 0 for k in ("scene_rgba_grad", "scene_dist_grad")), "cotangents on rgb, alpha and hit distance"


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_response_and_its_gradient_bit_for_bit(golden, units, degree):
    resp, grad = run_responses(units, degree, golden)
    assert_bit_equal(resp, golden[f"resp{degree}"], f"particleResponse<{degree}>")
    assert_bit_equal(grad, golden[f"resp{degree}_grad"], f"particleResponseGrd<{degree}>")


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_per_hit_backward_step_bit_for_bit(golden, units, degree):
    got = run_hit_cases(units, degree, golden)
    for name in ("accepted", "state_after", "density_grad", "feat_grad"):
        assert_bit_equal(got[name], golden[f"hit{degree}_{name}"], f"processHitBwd<{degree}> {name}")


@pytest.mark.parametrize("deg", range(4))
def test_sh_radiance_and_its_backward_bit_for_bit(golden, units, deg):
    cl, un, gr = run_sh(units, deg, golden)
    assert_bit_equal(cl, golden[f"sh{deg}_clamped"], f"radianceFromSpH({deg}) clamped")
    assert_bit_equal(un, golden[f"sh{deg}_unclamped"], f"radianceFromSpH({deg}) unclamped")
    # the oracle's backward multiplies in double (its cotangent is a double sum); for an fp32 cotangent that product is exact and
    # rounds to the reference's fp32 product
    assert gr.dtype == np.float64
    assert_bit_equal(gr.astype(np.float32), golden[f"sh{deg}_grad"], f"radianceFromSpHBwd({deg})")


def test_quaternion_to_rows_bit_for_bit(golden, units):
    assert_bit_equal(np.stack([units.quat_rows(q) for q in golden["quat"]]), golden["quat_rows"], "quaternionWXYZToMatrix")


def scene_view():
    return make_view("pinhole", rc.SCENE_W, rc.SCENE_H, cams.look_at_c2w(rc.SCENE_EYE, rc.SCENE_TARGET), fx=rc.SCENE_FX)


def worst_row_difference(got, want):
    nr = np.linalg.norm(want, axis=1)
    assert (nr > 0).all()
    return float((np.linalg.norm(got - want, axis=1) / nr).max())


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_backward_of_the_composed_scene_against_the_reference_sums(golden, degree):
    view = scene_view()
    prm = oracle.default_params(); prm.kernel_degree = degree
    d12, sph = golden["scene_d12"], golden["scene_sph"]
    fwd = oracle.forward(view["oracle_cam"], rc.SCENE_W, rc.SCENE_H, d12, sph, view["ro"], view["rd"], sh_degree=rc.SCENE_SH_DEGREE, params=prm)
    dens_g, sph_g, _ = oracle.backward(view["oracle_cam"], fwd, golden["scene_rgba_grad"], golden["scene_dist_grad"], params=prm)
    assert not dens_g[:, 11].any()
    # the forward (the restated Slang hit) and the reference's backward accept the same (ray, entry) pairs on this scene: every Gaussian
    # lies in front of the camera, so the forward's hit-distance window, which the backward does not have, rejects nothing
    assert int(fwd["hits"].sum()) == int(golden[f"scene{degree}_pairs"])
    e12 = worst_row_difference(dens_g, golden[f"scene{degree}_g12"])
    e48 = worst_row_difference(sph_g, golden[f"scene{degree}_g48"])
    print(f"[scene, degree {degree}] worst relative row difference: [12,12] {e12:.3g}, [12,48] {e48:.3g}; {int(golden[f'scene{degree}_pairs'])} accepted pairs")
    assert e12 <= 10 * SCENE_G12_MEASURED and e48 <= 10 * SCENE_G48_MEASURED, (e12, e48)


def test_fixture_is_what_the_reference_library_gives(golden):
    """Re-runs the fixture's inputs through oracle/_ref/libgut_refhits.so where the reference tree was at hand to build it."""
    ref = oracle.HitUnits.reference()
    if ref is None:
        pytest.skip("oracle/_ref/libgut_refhits.so is not built (no reference tree beside the repository)")
    for n in rc.DEGREES:
        got = run_hit_cases(ref, n, golden)
        for name in ("accepted", "state_after", "density_grad", "feat_grad"):
            assert_bit_equal(got[name], golden[f"hit{n}_{name}"], f"reference processHitBwd<{n}> {name}")
        resp, grad = run_responses(ref, n, golden)
        assert_bit_equal(resp, golden[f"resp{n}"], f"reference particleResponse<{n}>")
        assert_bit_equal(grad, golden[f"resp{n}_grad"], f"reference particleResponseGrd<{n}>")
    for deg in range(4):
        cl, un, gr = run_sh(ref, deg, golden)
        assert_bit_equal(cl, golden[f"sh{deg}_clamped"], "reference radianceFromSpH clamped")
        assert_bit_equal(un, golden[f"sh{deg}_unclamped"], "reference radianceFromSpH unclamped")
        assert_bit_equal(gr, golden[f"sh{deg}_grad"], "reference radianceFromSpHBwd")
    assert_bit_equal(np.stack([ref.quat_rows(q) for q in golden["quat"]]), golden["quat_rows"], "reference quaternionWXYZToMatrix")
