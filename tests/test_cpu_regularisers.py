"""CPU tests of the MCMC regularisers' host side: the reference's `loss:` blocks -> trainer arguments, the torch restatement's
gradient against the closed form the kernels implement, and the C ABI of GutRegularisation."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = importlib.import_module("3dgrut_amd._capi")
losses = importlib.import_module("3dgrut_amd.losses")
strategy = importlib.import_module("3dgrut_amd.strategy")

# configs/base_gs.yaml:111-126 and configs/base_mcmc.yaml:13-18 (which overrides base_gs), as plain dicts
BASE_GS_LOSS = dict(use_l1=True, lambda_l1=0.8, use_l2=False, lambda_l2=1.0, use_ssim=True, lambda_ssim=0.2,
                    use_opacity=False, lambda_opacity=0.0, use_scale=False, lambda_scale=0.0)
BASE_MCMC_LOSS = dict(BASE_GS_LOSS, use_opacity=True, lambda_opacity=0.01, use_scale=True, lambda_scale=0.01)


def test_loss_weights_of_the_reference_configs():
    assert losses.loss_weights(BASE_GS_LOSS) == dict(lambda_l1=0.8, lambda_ssim=0.2, lambda_opacity=0.0, lambda_scale=0.0)
    assert losses.loss_weights(BASE_MCMC_LOSS) == dict(lambda_l1=0.8, lambda_ssim=0.2, lambda_opacity=0.01, lambda_scale=0.01)
    w = losses.loss_weights(BASE_MCMC_LOSS)
    assert {k: w[k] for k in strategy.MCMC_LOSS} == strategy.MCMC_LOSS


def test_loss_weights_honour_the_use_switches_and_ignore_l2():
    off = dict(BASE_MCMC_LOSS, use_l1=False, use_ssim=False, use_opacity=False, use_scale=False)
    assert losses.loss_weights(off) == dict(lambda_l1=0.0, lambda_ssim=0.0, lambda_opacity=0.0, lambda_scale=0.0)
    # trainer.py:449 sums L1, SSIM, opacity and scale: the L2 term is computed but never enters the total loss
    with_l2 = dict(BASE_GS_LOSS, use_l2=True, lambda_l2=5.0)
    assert losses.loss_weights(with_l2) == losses.loss_weights(BASE_GS_LOSS)
    assert "lambda_l2" not in losses.loss_weights(with_l2)
    assert losses.loss_weights(dict(lambda_opacity=0.5)) == dict(lambda_l1=0.0, lambda_ssim=0.0, lambda_opacity=0.0, lambda_scale=0.0)


def test_regularisation_loss_gradient_is_the_closed_form():
    g = torch.Generator().manual_seed(0)
    n = 257
    d = (torch.randn((n, 1), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    s = (torch.randn((n, 3), generator=g, dtype=torch.float64) - 3).requires_grad_(True)
    lo, ls = 0.01, 0.7
    o, sc = losses.regularisation_loss(torch.sigmoid(d), torch.exp(s), lo, ls)
    assert torch.allclose(o, lo * torch.sigmoid(d).mean()) and torch.allclose(sc, ls * torch.exp(s).mean())
    (o + sc).backward()
    sig = torch.sigmoid(d.detach())
    assert torch.allclose(d.grad, (lo / n) * sig * (1 - sig), rtol=1e-12, atol=0)
    assert torch.allclose(s.grad, (ls / (3 * n)) * torch.exp(s.detach()), rtol=1e-12, atol=0)


def test_gut_regularisation_mirror_matches_the_compiled_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "reg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gut_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(GutRegularisation), offsetof(GutRegularisation, density_coeff), offsetof(GutRegularisation, scale_coeff), '
                   'offsetof(GutRegularisation, d_partials), GUT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "reg"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = capi.GutRegularisation
    assert got == [C.sizeof(R), R.density_coeff.offset, R.scale_coeff.offset, R.d_partials.offset, capi.GUT_ABI_VERSION], got
    assert capi.GUT_ABI_VERSION == 6


def test_regularisation_symbols_are_exported():
    lib = capi.load()
    for sym in ("gut_set_regularisation", "gut_sh_adam_step_regularised", "gut_adam_unwalked_waves_regularised", "gut_sync_moments_ex",
                "gut_regularisation_gradient", "gut_regularisation_loss"):
        assert sym in capi.EXPORTS and hasattr(lib, sym), sym
    # the handle setter checks its handle before anything else: an error, without a GPU
    assert lib.gut_set_regularisation(None, None) != 0


def test_trainers_take_the_regularisers():
    import inspect
    native = importlib.import_module("3dgrut_amd.native")
    train = importlib.import_module("3dgrut_amd.train")
    for cls in (native.NativeTrainStep, train.TrainStep):
        p = inspect.signature(cls.__init__).parameters
        assert p["lambda_opacity"].default == 0.0 and p["lambda_scale"].default == 0.0, cls
