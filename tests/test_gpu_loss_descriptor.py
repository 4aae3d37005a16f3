"""gut_photometric_loss_run, the descriptor form of the fused loss, against the positional entry point of the same operands: the
same function behind both, so every output is asked to be BIT-equal — loss3, d rgba and, with an exposure, dE — for all eight
combinations of mask x background (constant white / plane) x exposure, plus constant black alone.  Outputs start NaN-filled: equal
bits to a finite result also say every element was written.  Inputs and the positional calls are those of
tests/test_gpu_exposure_loss.py (whose own tests hold the positional forms to the fp64 reference)."""
import ctypes as C
import importlib

import pytest
import torch

from tests.test_gpu_exposure_loss import MASK_SHAPES, SHAPES, _call, _case, _dev, _existing, bits

pytestmark = pytest.mark.gpu
capi = importlib.import_module("3dgrut_amd._capi")

# partial tiles both ways, more than one tile; a single tile with one valid SSIM row (unmasked only: _mask needs a width above 45)
BIG, SMALL = SHAPES[0], SHAPES[2]
assert BIG == (37, 53) and SMALL == (12, 17) and BIG in MASK_SHAPES
CASES = [(BIG, bg, masked, exp) for bg in ("white", "plane") for masked in (False, True) for exp in (False, True)] \
    + [(SMALL, bg, False, exp) for bg in ("white", "plane") for exp in (False, True)] \
    + [(BIG, "black", False, False), (SMALL, "black", False, False)]


def _run(H, W, d, with_exposure, want_dE=True, ws=None):
    """One call of gut_photometric_loss_run on the device tensors of _dev() into NaN-filled outputs."""
    lib = capi.load()
    if ws is None:
        size = lib.gut_photometric_exposure_workspace_bytes(H, W) if with_exposure else lib.gut_photometric_workspace_bytes(H, W)
        ws = torch.empty(((size + 3) // 4,), dtype=torch.float32, device="cuda")
    out3 = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
    dE = torch.full((12,), float("nan"), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    desc = capi.GutPhotometricLoss(d_rgba=d["rgba"].data_ptr(), d_gt_rgb=d["gt"].data_ptr(), d_mask=ptr(d["mask"]), d_background=ptr(d["B"]),
                                   d_exposure12=d["E"].data_ptr() if with_exposure else None, d_workspace=ws.data_ptr(),
                                   d_loss3=out3.data_ptr(), d_rgba_grad=grad.data_ptr(),
                                   d_exposure_grad12=dE.data_ptr() if with_exposure and want_dE else None,
                                   background=d["bg"], lambda_l1=0.8, lambda_ssim=0.2)
    rc = lib.gut_photometric_loss_run(C.c_void_p(torch.cuda.current_stream().cuda_stream), H, W, C.byref(desc))
    assert rc == 0
    torch.cuda.synchronize()
    return out3, grad, dE


@pytest.mark.parametrize("hw,background,masked,with_exposure", CASES)
def test_descriptor_call_gives_the_bits_of_the_positional_entry_point(hw, background, masked, with_exposure):
    H, W = hw
    d = _dev(_case(H, W, background, masked))
    new3, newg, newE = _run(H, W, d, with_exposure)
    if with_exposure:
        old3, oldg, oldE = _call(H, W, **d)
        assert torch.isfinite(newE).all() and torch.equal(bits(newE), bits(oldE))
    else:
        old3, oldg = _existing(H, W, d)
        assert bool(torch.isnan(newE).all())                      # no exposure: nothing is written there
    assert torch.isfinite(new3).all() and torch.isfinite(newg).all()   # every output element was written
    assert torch.equal(bits(new3), bits(old3)) and torch.equal(bits(newg), bits(oldg))


@pytest.mark.parametrize("background,masked", [("plane", True), ("black", False)])
def test_null_gradient_output_applies_the_exposure_and_reduces_nothing(background, masked):
    H, W = BIG
    d = _dev(_case(H, W, background, masked))
    lib = capi.load()
    ws = torch.full(((lib.gut_photometric_exposure_workspace_bytes(H, W) + 3) // 4,), 7.0, dtype=torch.float32, device="cuda")
    base_words = (lib.gut_photometric_workspace_bytes(H, W) + 3) // 4
    n3, ng, sentinel = _run(H, W, d, True, want_dE=False, ws=ws)
    assert bool(torch.isnan(sentinel).all())                    # the 12 floats that WOULD have been the output: untouched
    assert bool((ws[base_words:] == 7.0).all())                 # no partial was written either
    w3, wg, wE = _run(H, W, d, True, ws=ws)
    assert torch.isfinite(wE).all() and not bool((ws[base_words:base_words + 12] == 7.0).all())
    assert torch.equal(bits(n3), bits(w3)) and torch.equal(bits(ng), bits(wg))
    assert torch.isfinite(ng).all()
