"""gut_image_metrics_cc (losses.image_metrics_colour_corrected) on the GPU against the float64 yardstick of
tests/cc_reference.py — an augmented least-squares fit, a float64 image, train.ssim in double — never against the code under test.

Bars.  The fitted E: 1e-6 absolute per entry (sixteen fp32 ulps at the largest entry, 1.2): the kernel differs from the float64 fit
by the fp32 rounding of its twelve outputs (<= 7e-8) and the order of its double sums (<= 1e-12 on these inputs); the reference's
cond(G) <= 1e4 is asserted so that the bar stays meaningful.  The four metrics: those of tests/test_gpu_metrics.py (MSE relative 1e-6,
PSNR 1e-4 dB, SSIM and L1 2e-6); MSE is first-order insensitive to the error of E at the optimum.  The exact-affine bound is
derived: the objective at the fitted E is at most the objective at the true one, so MSE_cc <= ridge |E* - [I | 0]|_F^2 / 3.

Measured on MI355X over the twenty cases: max |E - E64| 1.9e-8 .. 5.2e-8, MSE relative <= 1.1e-7, PSNR <= 8.9e-7 dB, SSIM <= 2.0e-7,
L1 <= 3.4e-9; exact affine: corrected MSE 2.4e-13, |E - E_TEST| 2.1e-6, plain PSNR 19.6 dB."""
import ctypes as C
import functools
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cc_reference as ref
from tests.synthetic_colmap import write_synthetic_colmap

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")
evaluate_mod = importlib.import_module("3dgrut_amd.evaluate")
io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
capi = importlib.import_module("3dgrut_amd._capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _reference(H, W, kind, background):
    """The float64 yardstick of one case, computed once: (E, cond(G), (MSE, PSNR, SSIM, L1) corrected, plain MSE)."""
    rgba, gt = ref.images(H, W, kind, background)
    comp = ref.composite(rgba, background)
    E, cond = ref.reference_fit(comp, gt)
    window = train._gauss_window(dtype=torch.float64)
    return E, cond, ref.reference_metrics(comp, gt, E, train.ssim, window), ref.sse(comp, gt, ref.IDENTITY34) / (3 * H * W)


def _raw_call(rgba, gt, bg, ridge, out4, e12):
    """The C entry point itself (e12 may be None: d_exposure12 = NULL)."""
    lib = capi.load()
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    ws = torch.empty(((lib.gut_image_metrics_cc_workspace_bytes(H, W) + 7) // 8,), dtype=torch.float64, device=rgba.device)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    rc = lib.gut_image_metrics_cc(C.c_void_p(stream), H, W, rgba.data_ptr(), gt.data_ptr(), bg, ridge, ws.data_ptr(), out4.data_ptr(),
                                  None if e12 is None else e12.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return out4


@pytest.mark.parametrize("background", ref.BACKGROUNDS)
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("hw", ref.SHAPES)
def test_fit_and_corrected_metrics_match_float64(hw, kind, background):
    H, W = hw
    rgba, gt = ref.images(H, W, kind, background)
    E_ref, cond, (mse, psnr, ssim, l1), plain_mse = _reference(H, W, kind, background)
    assert cond <= 1e4, cond                                             # on the reference alone: the 1e-6 bar stays meaningful
    d_rgba, d_gt = rgba.cuda(), gt.cuda()
    out = torch.full((4,), float("nan"), device="cuda")
    E = torch.full((3, 4), float("nan"), device="cuda")
    got_out, got_E = losses.image_metrics_colour_corrected(d_rgba, d_gt, background=background, ridge=ref.RIDGE, out=out, exposure_out=E)
    assert got_out.data_ptr() == out.data_ptr() and got_E.data_ptr() == E.data_ptr() and tuple(got_E.shape) == (3, 4)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(E).all())   # every element was written
    e = E.cpu().double().numpy()
    m = out.cpu().double().numpy()
    err_E = float(np.abs(e - E_ref).max())
    print(f"\n[cc {H}x{W} {kind} {background}] cond(G) {cond:.3g}; max |E - E64| {err_E:.3e}; MSE rel {abs(m[0] - mse) / mse:.3e}, "
          f"PSNR {abs(m[1] - psnr):.3e} dB, SSIM {abs(m[2] - ssim):.3e}, L1 {abs(m[3] - l1):.3e}; cc MSE {m[0]:.6e}, plain {plain_mse:.6e}")
    assert err_E <= 1e-6, err_E
    assert abs(m[0] - mse) <= 1e-6 * mse, (m[0], mse)
    assert abs(m[1] - psnr) <= 1e-4, (m[1], psnr)
    assert abs(m[2] - ssim) <= 2e-6, (m[2], ssim)
    assert abs(m[3] - l1) <= 2e-6, (m[3], l1)
    # exact properties: identical bits on a second call, with and without d_exposure12, and the corrected MSE never above the plain
    out2, E2 = losses.image_metrics_colour_corrected(d_rgba, d_gt, background=background, ridge=ref.RIDGE)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(E2.view(torch.int32), E.view(torch.int32))
    bg = 1.0 if background == "white" else 0.0
    out3 = _raw_call(d_rgba, d_gt, bg, ref.RIDGE, torch.full((4,), float("nan"), device="cuda"), None)
    assert torch.equal(out3.view(torch.int32), out.view(torch.int32))
    plain = losses.image_metrics(d_rgba, d_gt, background=background).cpu().double().numpy()
    assert m[0] <= plain[0] * (1.0 + 1e-6), (m[0], plain[0])
    assert abs(plain[0] - plain_mse) <= 1e-6 * plain_mse


def test_exact_affine_is_recovered_within_the_ridge_bound():
    """gt = fp32(E_TEST comp), no noise, 37 x 53 over black: corrected MSE within the derived bound (2.5e-8) + 1e-12 (the float64
    restatement gives 2.5e-13), E within 1e-5 of E_TEST (the ridge's bias is 2.1e-6), while the plain PSNR stays below 25 dB."""
    rgba, gt = ref.images(37, 53, "iid", "black", noise=0.0)
    out, E = losses.image_metrics_colour_corrected(rgba.cuda(), gt.cuda(), ridge=ref.RIDGE)
    plain = losses.image_metrics(rgba.cuda(), gt.cuda())
    bound = ref.ridge_bound(ref.E_TEST)
    err = float(np.abs(E.cpu().double().numpy() - ref.E_TEST).max())
    print(f"\n[cc exact affine] corrected MSE {float(out[0]):.3e} (bound {bound:.3e}), plain PSNR {float(plain[1]):.2f} dB, max |E - E_TEST| {err:.3e}")
    assert bound == pytest.approx(2.48e-8, rel=1e-3)
    assert float(out[0]) <= bound + 1e-12
    assert float(plain[1]) < 25.0
    assert err <= 1e-5


def test_identity_when_the_image_is_the_photo():
    rgba, _ = ref.images(37, 53, "iid", "white")
    gt = ref.composite(rgba, "white").contiguous()
    out, E = losses.image_metrics_colour_corrected(rgba.cuda(), gt.cuda(), background="white", ridge=ref.RIDGE)
    assert float((E.cpu().double() - torch.as_tensor(ref.IDENTITY34)).abs().max()) <= 1e-6
    assert 0.0 <= float(out[0]) <= 1e-12


def test_neighbours_stay_untouched_and_arguments_are_checked():
    rgba, gt = ref.images(40, 56, "correlated", "black")
    d_rgba, d_gt = rgba.cuda(), gt.cuda()
    before = losses.image_metrics(d_rgba, d_gt)
    rows4 = torch.full((3, 4), float("nan"), device="cuda")
    rows12 = torch.full((3, 12), float("nan"), device="cuda")
    out, E = losses.image_metrics_colour_corrected(d_rgba, d_gt, out=rows4[1], exposure_out=rows12[1])
    assert tuple(E.shape) == (3, 4) and E.data_ptr() == rows12[1].data_ptr()
    for rows in (rows4, rows12):       # a row of a [V,4] / [V,12] tensor; the other rows untouched
        assert bool(torch.isfinite(rows[1]).all()) and bool(torch.isnan(rows[0]).all()) and bool(torch.isnan(rows[2]).all())
    after = losses.image_metrics(d_rgba, d_gt)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    # [1,H,W,*] inputs as evaluate() has them
    out1, E1 = losses.image_metrics_colour_corrected(d_rgba[None], d_gt[None])
    assert torch.equal(out1, rows4[1]) and torch.equal(E1.reshape(12), rows12[1])
    a, b = torch.rand((10, 64, 4), device="cuda"), torch.rand((10, 64, 3), device="cuda")
    with pytest.raises(RuntimeError, match="10x10"):
        losses.image_metrics_colour_corrected(a, b)
    with pytest.raises(RuntimeError, match="exposure_out"):
        losses.image_metrics_colour_corrected(d_rgba, d_gt, exposure_out=torch.zeros((4, 3), device="cuda"))
    with pytest.raises(RuntimeError, match="out must"):
        losses.image_metrics_colour_corrected(d_rgba, d_gt, out=torch.zeros((3,), device="cuda"))
    # the torch restatement accepts device tensors and agrees with the kernel's fit
    E64 = losses.colour_correction(ref.composite(d_rgba, "black"), d_gt)
    assert E64.is_cuda and E64.dtype == torch.float64 and float((E64 - rows12[1].reshape(3, 4).double()).abs().max()) <= 1e-6


def test_evaluate_scores_every_view_through_its_own_fit(gut, tmp_path):
    """The model, tracer and five 96 x 96 views of tests/test_gpu_metrics.py::test_evaluate_aggregates_its_per_view_metrics; each
    view's photo is its own render passed through a seeded affine (gains in [0.8, 1.2], offsets in [-0.02, 0.02]), so the corrected
    MSE of view i is at most the ridge bound of its affine."""
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    native = importlib.import_module("3dgrut_amd.native")
    model = native.NativeGaussianModel(scenes.scene_c1(3000, 5), device="cuda")
    tracer = gut.Tracer({"render": {}})
    W = H = 96
    ro, rd = cams.pinhole_rays(W, H, 90.0, 90.0)
    K = cams.pinhole_intrinsics_dict(W, H, 90.0, 90.0)
    g = torch.Generator().manual_seed(9)
    affines, batches = [], []
    for i in range(5):
        b = gut.Batch(rays_ori=torch.as_tensor(ro, device="cuda"), rays_dir=torch.as_tensor(rd, device="cuda"),
                      T_to_world=torch.as_tensor(cams.orbit_c2w(4.0, 40.0 * i, 15.0), device="cuda")[None],
                      rgb_gt=torch.zeros((1, H, W, 3), device="cuda"), intrinsics_OpenCVPinholeCameraModelParameters=K)
        E = torch.cat([torch.diag(0.8 + 0.4 * torch.rand((3,), generator=g)), 0.04 * torch.rand((3, 1), generator=g) - 0.02], dim=1)
        with torch.no_grad():
            render = tracer.render(model, b, train=False)["pred_rgb"].contiguous()
            b.rgb_gt = losses.apply_exposure(render, E.cuda()).contiguous()
        affines.append(E.double().numpy())
        batches.append(b)
    off = evaluate_mod.evaluate(model, tracer, batches)
    assert not any(k.startswith("cc_") or "_cc_" in k for k in off)
    on = evaluate_mod.evaluate(model, tracer, batches, out_dir=str(tmp_path), step=7, colour_corrected=True, ridge=ref.RIDGE)
    assert set(on) - set(off) == {"cc_psnr", "cc_ssim", "cc_mse", "cc_l1", "mean_cc_psnr", "std_cc_psnr", "mean_cc_ssim", "cc_transforms"}
    assert on["psnr"] == off["psnr"] and on["ssim"] == off["ssim"] and on["mse"] == off["mse"] and on["l1"] == off["l1"]
    print(f"\n[cc evaluate] plain psnr {[round(x, 2) for x in on['psnr']]}, corrected mse {on['cc_mse']}, bounds "
          f"{[ref.ridge_bound(E) for E in affines]}")
    for i, E in enumerate(affines):
        assert on["cc_mse"][i] <= ref.ridge_bound(E) + 1e-12, (i, on["cc_mse"][i])
    assert np.asarray(on["cc_transforms"]).shape == (5, 3, 4)
    assert on["mean_cc_psnr"] == pytest.approx(float(np.mean(on["cc_psnr"])), abs=1e-9)
    assert on["std_cc_psnr"] == pytest.approx(float(np.std(on["cc_psnr"])), abs=1e-9)
    assert on["mean_cc_ssim"] == pytest.approx(float(np.mean(on["cc_ssim"])), abs=1e-9)
    for i in range(5):
        assert os.path.isfile(os.path.join(str(tmp_path), "ours_7", "renders", f"{i:05d}.png"))
        assert os.path.isfile(os.path.join(str(tmp_path), "ours_7", "renders_cc", f"{i:05d}.png"))
    with pytest.raises(ValueError, match="ridge"):
        evaluate_mod.evaluate(model, tracer, batches, colour_corrected=True, ridge=0.0)


# ---- a short run through the command line ----
def _cli(args, timeout=300):
    r = subprocess.run([sys.executable, "-m", "3dgrut_amd.trainer"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return r, json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None


def test_short_run_reports_colour_corrected_scores_through_the_cli(tmp_path):
    """The reduced synthetic COLMAP scene of tests/test_gpu_exposure_training.py (16 views of 160 x 160, every 8th held out), 60
    steps (no densification event needed: the run only has to reach its final evaluation), whose TEST images are multiplied by a
    per-view gain in [0.8, 1.2]: with --exposure --cc-metrics the final JSON holds the corrected means, and the corrected PSNR is not
    below the plain one (SSE(E) <= SSE(I) per view; 1e-4 dB is the PSNR bar above).  Without --cc-metrics the `test` dictionary has
    exactly the keys it had.  The gain in dB is printed, not asserted: nothing predicts it."""
    from PIL import Image
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=16, size=160, n_teacher=40_000, n_points=4_000)
    test = io_colmap.ColmapScene(root, "test", 1, 8)
    g = torch.Generator().manual_seed(4)
    gains = 0.8 + 0.4 * torch.rand((len(test.images),), generator=g, dtype=torch.float64)
    gains = (gains / gains.log().mean().exp()).numpy()
    for im, gain in zip(test.images, gains):
        path = os.path.join(root, "images", im.name)
        with Image.open(path) as img:
            px = np.asarray(img.convert("RGB"), np.float64) / 255.0
        Image.fromarray((np.clip(px * gain, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)).save(path)
    out_c, out_p = str(tmp_path / "cc"), str(tmp_path / "plain")
    r, with_cc = _cli(["--path", root, "--n-iterations", "60", "--out-dir", out_c, "--exposure", "--cc-metrics"])
    assert r.returncode == 0, r.stderr[-2000:]
    r, without = _cli(["--path", root, "--n-iterations", "60", "--out-dir", out_p, "--exposure"])
    assert r.returncode == 0, r.stderr[-2000:]
    t = with_cc["test"]
    print(f"\n[cc run] held-out gains {[round(float(x), 3) for x in gains]}: plain psnr {t['mean_psnr']:.3f} dB, colour-corrected "
          f"{t['mean_cc_psnr']:.3f} +- {t['std_cc_psnr']:.3f} dB (gain {t['mean_cc_psnr'] - t['mean_psnr']:.3f} dB); ssim "
          f"{t['mean_ssim']:.4f} -> {t['mean_cc_ssim']:.4f}")
    assert set(t) == {"mean_psnr", "std_psnr", "mean_ssim", "n_views", "mean_cc_psnr", "std_cc_psnr", "mean_cc_ssim"}
    assert set(without["test"]) == {"mean_psnr", "std_psnr", "mean_ssim", "n_views"}
    assert with_cc["stats"]["n_steps"] == 60 and t["n_views"] == len(gains)
    assert all(math.isfinite(t[k]) for k in t)
    assert t["mean_cc_psnr"] >= t["mean_psnr"] - 1e-4
    assert os.path.isfile(os.path.join(out_c, "ours_60", "renders_cc", "00000.png"))
    assert not os.path.exists(os.path.join(out_p, "ours_60", "renders_cc"))
