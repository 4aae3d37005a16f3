"""gut_image_metrics (losses.image_metrics) against a float64 torch restatement — composite, then MSE / PSNR, then train.ssim in
double — and evaluate()'s aggregation.  Tolerances: SSIM and L1 within 2e-6 (the bar of test_gpu_losses.py), MSE relative 1e-6,
PSNR within 1e-4 dB."""
import importlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
losses = importlib.import_module("3dgrut_amd.losses")
train = importlib.import_module("3dgrut_amd.train")
evaluate_mod = importlib.import_module("3dgrut_amd.evaluate")


def _images(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rgba = torch.rand((H, W, 4), generator=g) * 1.4 - 0.2            # values outside [0, 1] too: the metrics are unclamped
    gt = (rgba[..., :3] + 0.3 * torch.randn((H, W, 3), generator=g)).clamp(-0.1, 1.1)
    return rgba, gt


@pytest.mark.parametrize("background", ["black", "white"])
@pytest.mark.parametrize("hw", [(11, 11), (37, 129), (800, 800), (1237, 822)])
def test_image_metrics_match_float64(background, hw):
    H, W = hw
    rgba, gt = _images(H, W, H * 7 + W)
    bg = 1.0 if background == "white" else 0.0
    out = losses.image_metrics(rgba.cuda(), gt.cuda(), background=background)
    got = out.cpu().double().numpy()
    img = (rgba[..., :3] + bg * (1.0 - rgba[..., 3:])).double()      # composited in fp32 as the kernel and BackgroundColor do
    g64 = gt.double()
    mse = float(((img - g64) ** 2).mean())
    ssim = float(train.ssim(img.permute(2, 0, 1)[None], g64.permute(2, 0, 1)[None], window=train._gauss_window(dtype=torch.float64)))
    l1 = float((img - g64).abs().mean())
    assert abs(got[0] - mse) <= 1e-6 * mse, (got[0], mse)
    assert abs(got[1] - 10.0 * math.log10(1.0 / mse)) <= 1e-4
    assert abs(got[2] - ssim) <= 2e-6, (got[2], ssim)
    assert abs(got[3] - l1) <= 2e-6
    again = losses.image_metrics(rgba.cuda(), gt.cuda(), background=background)
    assert torch.equal(out, again)   # fixed summation order: identical bits


def test_image_metrics_identical_images_and_refusals():
    rgba, _ = _images(40, 56, 1)
    rgba[..., 3] = 1.0
    out = losses.image_metrics(rgba.cuda(), rgba[..., :3].contiguous().cuda()).cpu()
    assert float(out[0]) == 0.0 and math.isinf(float(out[1])) and float(out[1]) > 0 and abs(float(out[2]) - 1.0) <= 1e-6
    rows = torch.full((3, 4), float("nan"), device="cuda")
    a, b = _images(24, 30, 2)
    losses.image_metrics(a.cuda(), b.cuda(), out=rows[1])   # a row of a [V,4] tensor; the other rows untouched
    assert torch.isfinite(rows[1]).all() and torch.isnan(rows[0]).all() and torch.isnan(rows[2]).all()
    a, b = _images(10, 64, 3)
    with pytest.raises(RuntimeError, match="10x10"):
        losses.image_metrics(a.cuda(), b.cuda())


def test_evaluate_aggregates_its_per_view_metrics(gut):
    scenes = importlib.import_module("3dgrut_amd.scenes")
    cams = importlib.import_module("3dgrut_amd.cameras")
    native = importlib.import_module("3dgrut_amd.native")
    model = native.NativeGaussianModel(scenes.scene_c1(3000, 5), device="cuda")
    tracer = gut.Tracer({"render": {"enable_kernel_timings": True}})
    W = H = 96
    ro, rd = cams.pinhole_rays(W, H, 90.0, 90.0)
    K = cams.pinhole_intrinsics_dict(W, H, 90.0, 90.0)
    g = torch.Generator().manual_seed(9)
    batches = [gut.Batch(rays_ori=torch.as_tensor(ro, device="cuda"), rays_dir=torch.as_tensor(rd, device="cuda"),
                         T_to_world=torch.as_tensor(cams.orbit_c2w(4.0, 40.0 * i, 15.0), device="cuda")[None],
                         rgb_gt=torch.rand((1, H, W, 3), generator=g).cuda(), intrinsics_OpenCVPinholeCameraModelParameters=K)
               for i in range(5)]
    res = evaluate_mod.evaluate(model, tracer, batches)
    assert res["n_views"] == 5 and len(res["psnr"]) == 5 and len(res["ssim"]) == 5
    assert res["mean_psnr"] == pytest.approx(float(np.mean(res["psnr"])), abs=1e-9)
    assert res["std_psnr"] == pytest.approx(float(np.std(res["psnr"])), abs=1e-9)
    assert res["mean_ssim"] == pytest.approx(float(np.mean(res["ssim"])), abs=1e-9)
    assert res["mean_inference_time"] > 0
    with torch.no_grad():   # view 2 restated: the tracer's composited image against its ground truth
        pred = tracer.render(model, batches[2], train=False)["pred_rgb"][0].double()
    mse = float(((pred - batches[2].rgb_gt[0].double()) ** 2).mean())
    assert abs(res["psnr"][2] - 10.0 * math.log10(1.0 / mse)) <= 1e-4
    plain = evaluate_mod.evaluate(model, gut.Tracer({"render": {}}), batches)
    assert "mean_inference_time" not in plain
