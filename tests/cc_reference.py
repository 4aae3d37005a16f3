"""Inputs and the float64 yardstick of the colour-corrected metrics, shared by tests/test_cpu_cc_metrics.py and
tests/test_gpu_cc_metrics.py.  The reference fit is an AUGMENTED least-squares solve (numpy.linalg.lstsq on the stacked rows), not
the normal equations the kernels and losses.colour_correction use; nothing here calls the code under test."""
import functools

import numpy as np
import torch

# the matrix of tests/test_gpu_exposure_loss.py
E_TEST = np.array([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.03], [0.02, -0.05, 1.20, 0.04]], dtype=np.float64)
IDENTITY34 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
RIDGE = 1e-6
# (11, 11): the smallest accepted image, one partial workgroup of the moment pass; (37, 53): two workgroups, ragged; (520, 515): 262
# rows of partial moments, so the solve kernel's stride loop wraps
SHAPES = [(11, 11), (12, 17), (37, 53), (40, 56), (520, 515)]
KINDS = ["iid", "correlated"]
BACKGROUNDS = ["black", "white"]


def composite(rgba, background):
    """comp = rgb + background * (1 - alpha) in fp32, as composite3 and BackgroundColor compute it (black: rgb itself)."""
    bg = 1.0 if background == "white" else 0.0
    rgb = rgba[..., :3]
    return rgb if bg == 0.0 else rgb + bg * (1.0 - rgba[..., 3:])


def apply_fp32(comp, E):
    """fp32(E [comp; 1]) for a float64 E: the products in double, rounded once."""
    E = torch.as_tensor(E, dtype=torch.float64)
    return (comp.double() @ E[:, :3].T + E[:, 3]).float()


@functools.lru_cache(maxsize=None)
def images(H, W, kind, background, noise=0.05):
    """(rgba [H,W,4], gt [H,W,3]) float32 host tensors, seeded by the case: rgba = rand, for `correlated` rgb = 0.9 l + 0.1 rgb with
    one l = rand(H,W,1) (cond(G) 2e3 - 6e3, the regime of real images); gt = fp32(E_TEST comp) + noise * randn."""
    g = torch.Generator().manual_seed(H * 1009 + W * 7 + (1 if kind == "correlated" else 0) + (2 if background == "white" else 0))
    rgba = torch.rand((H, W, 4), generator=g)
    if kind == "correlated":
        lum = torch.rand((H, W, 1), generator=g)
        rgba[..., :3] = 0.9 * lum + 0.1 * rgba[..., :3]
    comp = composite(rgba, background)
    gt = apply_fp32(comp, E_TEST)
    if noise:
        gt = gt + noise * torch.randn((H, W, 3), generator=g)
    return rgba.contiguous(), gt.contiguous()


def reference_fit(comp, gt, ridge=RIDGE):
    """(E [3,4], cond(G)) in float64: lstsq on [X; sqrt(ridge P) I_4] against [Y; sqrt(ridge P) [I_3; 0]], X = [comp, 1]."""
    x = comp.reshape(-1, 3).double().numpy()
    y = gt.reshape(-1, 3).double().numpy()
    P = x.shape[0]
    X = np.concatenate([x, np.ones((P, 1))], axis=1)
    r = np.sqrt(ridge * P)
    Xa = np.concatenate([X, r * np.eye(4)], axis=0)
    Ya = np.concatenate([y, r * np.eye(4)[:, :3]], axis=0)
    Et, *_ = np.linalg.lstsq(Xa, Ya, rcond=None)
    return Et.T.copy(), float(np.linalg.cond(Xa.T @ Xa))


def reference_metrics(comp, gt, E, ssim_fn, window):
    """(MSE, PSNR, SSIM, L1) in float64 of E [comp; 1] against gt: float64 image, `ssim_fn` (train.ssim) in double."""
    E = torch.as_tensor(E, dtype=torch.float64)
    img = comp.double() @ E[:, :3].T + E[:, 3]
    g64 = gt.double()
    mse = float(((img - g64) ** 2).mean())
    ssim = float(ssim_fn(img.permute(2, 0, 1)[None], g64.permute(2, 0, 1)[None], window=window))
    l1 = float((img - g64).abs().mean())
    psnr = 10.0 * np.log10(1.0 / mse) if mse > 0 else float("inf")
    return mse, psnr, ssim, l1


def sse(comp, gt, E):
    E = torch.as_tensor(E, dtype=torch.float64)
    return float((((comp.double() @ E[:, :3].T + E[:, 3]) - gt.double()) ** 2).sum())


def ridge_bound(E_true, ridge=RIDGE):
    """For gt = A* comp + b* exactly: MSE_cc <= ridge |[A* | b*] - [I | 0]|_F^2 / 3 (the objective at E is at most the one at E*)."""
    return ridge * float(((np.asarray(E_true, np.float64) - IDENTITY34) ** 2).sum()) / 3.0
