"""tests/loss_cases.py on the CPU alone: the float64 reference is the definition the older loss tests use, every case keeps its
decision margin, every bar is usable, a second float32 evaluation (the kernels' derivative-map scheme in torch) stays within half of
every bar, and the bars bite: each altered rule of VARIANTS, evaluated in float64, lands outside them — while the two that matter
most in training (C1, the subgradient at a tie) stay inside the fixed tolerances of the older white-noise tests.  No device."""
import importlib

import pytest
import torch

from tests import loss_cases as lc
from tests import test_gpu_exposure_loss as old

losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")

CASES = [(fam, hw, combo[0]) for fam in lc.FAMILIES for hw in lc.SHAPES for combo in lc.COMBOS]
KEYS = ("grad", "dE", "ssim", "l1", "loss")


@pytest.mark.parametrize("hw,background,masked", old.CASES)
def test_float64_reference_is_the_older_tests_definition(hw, background, masked):
    """On tests/test_gpu_exposure_loss.py's own inputs reference() gives what its _case gives: losses.photometric_loss with
    apply_exposure and train.ssim under float64 autograd."""
    H, W = hw
    c = old._case(H, W, background, masked)
    r = lc.reference(c["rgba"], c["gt"], background=c["B"] if c["B"] is not None else c["bg"], mask=c["mask"], exposure=old.E_TEST)
    assert abs(float(r["loss"]) - c["loss"]) <= 1e-15 and abs(float(r["l1"]) - c["l1"]) <= 1e-15 and abs(float(r["ssim"]) - c["ssim"]) <= 1e-14
    scale = float(c["grad"].abs().max())
    assert float((r["grad"] - c["grad"]).abs().max()) <= 1e-14 * scale
    assert float((r["dE"] - c["dE"]).abs().max()) <= 1e-14 * float(c["dE"].abs().max())
    img = r["p"].permute(2, 0, 1)[None]
    assert float(lc.ssim_map(img, r["q"].permute(2, 0, 1)[None]).mean()) == float(train.ssim(img, r["q"].permute(2, 0, 1)[None]))
    assert tuple(r["ssim_map"].shape) == (3, H - 10, W - 10) and tuple(r["abs_map"].shape) == (H, W, 3)


@pytest.mark.parametrize("fam,hw,combo", CASES)
def test_margin_bars_and_second_float32_evaluation(fam, hw, combo):
    H, W = hw
    c = lc.case(fam, H, W, combo)
    ops, b, r64 = c["ops"], c["bars"], c["r64"]
    # the decision margin: wherever the sign of p - q enters, |p - q| is exactly 0 or at least 1e-6, in float64 and float32 alike
    if ops["lambda_l1"] != 0.0:
        assert c["margin"] >= lc.MARGIN, c["margin"]
        assert bool(((c["r32"]["abs_map"] == 0) == (r64["abs_map"] == 0)).all())
    if fam in ("flat_ties", "identical") and ops["exposure"] is None:
        tied = (r64["abs_map"] == 0) & ((ops["mask"] if ops["mask"] is not None else torch.ones((H, W)))[..., None] != 0)
        assert int(tied.sum()) >= H * W // 2                                  # the ties are there, outside the mask's zeros too
    # the bars: finite; positive, except where the float64 map itself is zero everywhere and the check becomes the exact one
    exact_zero = not bool(r64["abs_map"].any())
    assert exact_zero == (fam == "identical" and ops["exposure"] is None)
    for k, v in b.items():
        if v is None:
            assert k == "dE" and ops["exposure"] is None
        elif exact_zero and k in ("l1", "mse"):
            assert v == 0.0 and not bool(c["r32"]["abs_map"].any())
        else:
            assert 0.0 < v < float("inf"), (k, v)
    # a correct float32 kernel has room: the derivative-map scheme in float32 torch stays within F / 2 of every bar
    got = lc.ratios(lc.scheme32(**ops), c)
    print(f"\n[{fam} {H}x{W} {combo}] margin {c['margin']:.2e}; bars " + ", ".join(f"{k} {v:.2e}" for k, v in b.items() if v is not None)
          + "; second float32 evaluation / bar " + ", ".join(f"{k} {v:.3f}" for k, v in got.items()))
    for k, v in got.items():
        assert v <= 0.5, (k, v)


def test_every_variant_breaks_the_bars():
    """Teeth: the float64 reference with one rule altered plays the kernel.  Printed: per variant and family, in how many of the
    family's 22 cases at least one output leaves its bar.  Every variant is caught somewhere; C1 swapped with C2 and the tie
    subgradient +1 are caught in every operand combination they apply to (the tie rule enters with lambda_l1 only, so not in the
    combinations with an exposure, where the two families that tie run on the SSIM term alone)."""
    table = {v: {f: 0 for f in lc.FAMILIES} for v in lc.VARIANTS}
    by_combo = {v: {c[0]: 0 for c in lc.COMBOS} for v in lc.VARIANTS}
    for fam, (H, W), combo in CASES:
        c = lc.case(fam, H, W, combo)
        for v in lc.VARIANTS:
            r = lc.ratios(lc.reference(**c["ops"], variant=v), c)
            if max(r.values()) > 1.0:
                table[v][fam] += 1
                by_combo[v][combo] += 1
    print("\ncases (of 22 per family) in which the variant leaves a bar\n" + " " * 18 + "".join(f"{f:>14}" for f in lc.FAMILIES))
    for v, row in table.items():
        print(f"{v:>18}" + "".join(f"{row[f]:>14}" for f in lc.FAMILIES))
    for v in lc.VARIANTS:
        assert sum(table[v].values()) > 0, v
    for combo, _, _, exposure in lc.COMBOS:
        assert by_combo["c1=9e-4"][combo] > 0, combo
        if not exposure:
            assert by_combo["tie=+1"][combo] > 0, combo
    assert sum(table["halo_mask=centre"].values()) == sum(by_combo["halo_mask=centre"][c[0]] for c in lc.COMBOS if c[2])   # masked cases only


def _opaque(img):
    """[3,H,W] -> rgba [H,W,4] with alpha 1."""
    return torch.cat([img.permute(1, 2, 0), torch.ones(img.shape[1:] + (1,))], -1)


@pytest.mark.parametrize("variant", ["c1=9e-4", "tie=+1"])
def test_the_older_tolerances_do_not_see_these_variants(variant):
    """The record of the gap: on the white-noise inputs of test_fused_ssim_matches_torch, test_fused_photometric_loss_and_gradient
    and test_photometric_loss_value (tests/test_gpu_losses.py, their small shapes) the altered definition stays within those tests'
    tolerances of the true one — 2e-6 on the SSIM, 1e-4 relative L2 on the gradient, 5e-6 on the loss — so a kernel that computed
    it would have passed them."""
    worst = dict(ssim=0.0, grad=0.0, loss=0.0)
    runs = []
    for shape in [(1, 3, 64, 80), (1, 3, 37, 53)]:                      # test_fused_ssim_matches_torch
        g = torch.Generator().manual_seed(5)
        a = torch.rand(shape, generator=g)
        b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
        runs.append(dict(rgba=_opaque(a[0]), gt=b[0].permute(1, 2, 0), lambda_l1=0.0, lambda_ssim=1.0))
    for H, W in [(40, 56), (37, 53)]:                                    # test_fused_photometric_loss_and_gradient
        for bg in (0.0, 1.0):
            g = torch.Generator().manual_seed(3)
            runs.append(dict(rgba=torch.rand((H, W, 4), generator=g), gt=torch.rand((H, W, 3), generator=g), background=bg))
    g = torch.Generator().manual_seed(1)                                 # test_photometric_loss_value
    runs.append(dict(rgba=_opaque(torch.rand((1, 40, 56, 3), generator=g)[0].permute(2, 0, 1)), gt=torch.rand((1, 40, 56, 3), generator=g)[0]))
    for ops in runs:
        base, alt = lc.reference(**ops), lc.reference(**ops, variant=variant)
        worst["ssim"] = max(worst["ssim"], abs(float(alt["ssim"] - base["ssim"])))
        worst["loss"] = max(worst["loss"], abs(float(alt["loss"] - base["loss"])))
        worst["grad"] = max(worst["grad"], float((alt["grad"] - base["grad"]).norm() / base["grad"].norm()))
    print(f"\n[{variant} on the older tests' inputs] largest shift: SSIM {worst['ssim']:.2e} (bar 2e-6), gradient rel-L2 {worst['grad']:.2e} "
          f"(bar 1e-4), loss {worst['loss']:.2e} (bar 5e-6)")
    assert worst["ssim"] <= 2e-6 and worst["grad"] <= 1e-4 and worst["loss"] <= 5e-6
