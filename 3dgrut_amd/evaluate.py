"""Held-out evaluation: the reference's `Renderer.render_all` (threedgrut/render.py:137-285) on this tree's tracer.

Every view is rendered with `Tracer.render(model, batch, train=False)` (a NativeGaussianModel or a GaussianModel) and scored on the
GPU by `losses.image_metrics` (csrc/gut_ssim.hip: gut_image_metrics) into one [V,4] device tensor that is read back once per pass.
The scored image is `outputs["pred_rgb"]`, already composited over the model's evaluation background (black or white; "random"
composites nothing at evaluation, i.e. black, as BackgroundColor does), unclamped, as the reference scores it.

PSNR is torchmetrics' PeakSignalNoiseRatio(data_range=1) of one image, SSIM equals StructuralSimilarityIndexMeasure(data_range=1)
(the valid-region mean: its reflect padding is cropped off again).  LPIPS is not provided: it needs the VGG weights of the `lpips`
package, which this project does not ship.
"""
import os

import numpy as np
import torch

from .losses import image_metrics


def _check_batch(batch, what):
    if getattr(batch, "rgb_gt", None) is None:
        raise ValueError(f"{what}: every batch needs rgb_gt")


def evaluate(model, tracer, batches, out_dir=None, step=0):
    """Render and score `batches`.  A batch's mask is ignored: every metric is of the full image, as in the reference, whose
    render.py and validation metrics never read the mask (it enters the training losses only).  Returns dict(psnr=[...],
    ssim=[...], mse=[...], l1=[...], mean_psnr, std_psnr (population std, as np.std), mean_ssim, n_views) and, when the tracer was
    built with render.enable_kernel_timings, mean_inference_time (ms per frame, the mean of the library's forward_render times).
    out_dir: the renders are written to out_dir/ours_{step}/renders/{i:05d}.png (clamped and rounded as torchvision.utils.save_image
    does)."""
    batches = list(batches)
    if not batches:
        raise ValueError("evaluate: no views")
    for b in batches:
        _check_batch(b, "evaluate")
    timed = bool(getattr(tracer.tracer_wrapper, "enable_kernel_timings", False))
    render_dir = None
    if out_dir:
        render_dir = os.path.join(out_dir, f"ours_{int(step)}", "renders")
        os.makedirs(render_dir, exist_ok=True)
    dev = batches[0].rays_ori.device
    metrics = torch.empty((len(batches), 4), dtype=torch.float32, device=dev)
    times = []
    with torch.no_grad():
        for i, batch in enumerate(batches):
            out = tracer.render(model, batch, train=False, frame_id=int(step))
            # the composited colour (the model's background applied by Tracer.render) and the opacity: nothing left to composite
            rgba = torch.cat([out["pred_rgb"][0], out["pred_opacity"][0]], dim=-1)
            image_metrics(rgba, batch.rgb_gt, background=0.0, out=metrics[i])
            if timed:
                times.append(float(out["frame_time_ms"]))
            if render_dir is not None:
                from PIL import Image
                img = out["pred_rgb"][0].mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy()
                Image.fromarray(img).save(os.path.join(render_dir, f"{i:05d}.png"))
    m = metrics.cpu().double().numpy()   # the pass's one device-to-host copy of the metrics
    psnr, ssim = m[:, 1], m[:, 2]
    res = dict(psnr=psnr.tolist(), ssim=ssim.tolist(), mse=m[:, 0].tolist(), l1=m[:, 3].tolist(), mean_psnr=float(np.mean(psnr)),
               std_psnr=float(np.std(psnr)), mean_ssim=float(np.mean(ssim)), n_views=len(batches))
    if timed:
        res["mean_inference_time"] = float(np.mean(times))
    return res
