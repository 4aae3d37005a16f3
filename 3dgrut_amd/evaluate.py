"""Held-out evaluation: the reference's `Renderer.render_all` (threedgrut/render.py:137-285) on this tree's tracer.

Every view is rendered with `Tracer.render(model, batch, train=False)` (a NativeGaussianModel or a GaussianModel) and scored on the
GPU by `losses.image_metrics` (csrc/gut_ssim.hip: gut_image_metrics) into one [V,4] device tensor that is read back once per pass.
The scored image is `outputs["pred_rgb"]`, already composited over the model's evaluation background (black or white; "random"
composites nothing at evaluation, i.e. black, as BackgroundColor does), unclamped, as the reference scores it.

PSNR is torchmetrics' PeakSignalNoiseRatio(data_range=1) of one image, SSIM equals StructuralSimilarityIndexMeasure(data_range=1)
(the valid-region mean: its reflect padding is cropped off again).  LPIPS is not provided: it needs the VGG weights of the `lpips`
package, which this project does not ship.

`colour_corrected=True` additionally scores every view COLOUR-CORRECTED (losses.image_metrics_colour_corrected):
the render is mapped through the affine colour transform that fits it best to the photo before it is scored, so that a held-out
photo's own exposure and white balance, which nothing in the model can absorb, are not charged to the model.  The fit runs on the
device as well; its metrics and transforms are read back together with the plain ones.
"""
import os

import numpy as np
import torch

from .losses import apply_exposure, image_metrics, image_metrics_colour_corrected


def _check_batch(batch, what):
    if getattr(batch, "rgb_gt", None) is None:
        raise ValueError(f"{what}: every batch needs rgb_gt")


def evaluate(model, tracer, batches, out_dir=None, step=0, colour_corrected=False, ridge=1e-6):
    """Render and score `batches`.  A batch's mask is ignored: every metric is of the full image, as in the reference, whose
    render.py and validation metrics never read the mask (it enters the training losses only).  Returns dict(psnr=[...],
    ssim=[...], mse=[...], l1=[...], mean_psnr, std_psnr (population std, as np.std), mean_ssim, n_views) and, when the tracer was
    built with render.enable_kernel_timings, mean_inference_time (ms per frame, the mean of the library's forward_render times).
    out_dir: the renders are written to out_dir/ours_{step}/renders/{i:05d}.png (clamped and rounded as torchvision.utils.save_image
    does).
    colour_corrected: every view is also scored through its fitted colour transform (ridge: the fit's regulariser, > 0); the plain
    metrics are the same calls and the same bits, and the result gains cc_psnr, cc_ssim, cc_mse, cc_l1 (lists), mean_cc_psnr,
    std_cc_psnr, mean_cc_ssim and cc_transforms ([V][3][4], the fitted [A | b] per view); with out_dir the corrected renders go to
    out_dir/ours_{step}/renders_cc/{i:05d}.png."""
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
        if colour_corrected:
            os.makedirs(os.path.join(out_dir, f"ours_{int(step)}", "renders_cc"), exist_ok=True)
    dev = batches[0].rays_ori.device
    metrics = torch.empty((len(batches), 4), dtype=torch.float32, device=dev)
    if colour_corrected:
        cc_metrics = torch.empty((len(batches), 4), dtype=torch.float32, device=dev)
        cc_transforms = torch.empty((len(batches), 12), dtype=torch.float32, device=dev)
    times = []
    with torch.no_grad():
        for i, batch in enumerate(batches):
            out = tracer.render(model, batch, train=False, frame_id=int(step))
            # the composited colour (the model's background applied by Tracer.render) and the opacity: nothing left to composite
            rgba = torch.cat([out["pred_rgb"][0], out["pred_opacity"][0]], dim=-1)
            image_metrics(rgba, batch.rgb_gt, background=0.0, out=metrics[i])
            if colour_corrected:
                image_metrics_colour_corrected(rgba, batch.rgb_gt, background=0.0, ridge=ridge, out=cc_metrics[i],
                                               exposure_out=cc_transforms[i])
            if timed:
                times.append(float(out["frame_time_ms"]))
            if render_dir is not None:
                from PIL import Image
                img = out["pred_rgb"][0].mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy()
                Image.fromarray(img).save(os.path.join(render_dir, f"{i:05d}.png"))
                if colour_corrected:
                    img = apply_exposure(out["pred_rgb"][0], cc_transforms[i]).mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy()
                    Image.fromarray(img).save(os.path.join(os.path.dirname(render_dir), "renders_cc", f"{i:05d}.png"))
    if colour_corrected:   # (one copy still: the three tensors side by side; the plain columns keep their bits)
        m = torch.cat([metrics, cc_metrics, cc_transforms], dim=1).cpu().double().numpy()
    else:
        m = metrics.cpu().double().numpy()   # the pass's one device-to-host copy of the metrics
    psnr, ssim = m[:, 1], m[:, 2]
    res = dict(psnr=psnr.tolist(), ssim=ssim.tolist(), mse=m[:, 0].tolist(), l1=m[:, 3].tolist(), mean_psnr=float(np.mean(psnr)),
               std_psnr=float(np.std(psnr)), mean_ssim=float(np.mean(ssim)), n_views=len(batches))
    if colour_corrected:
        cc_psnr, cc_ssim = m[:, 5], m[:, 6]
        res.update(cc_psnr=cc_psnr.tolist(), cc_ssim=cc_ssim.tolist(), cc_mse=m[:, 4].tolist(), cc_l1=m[:, 7].tolist(),
                   mean_cc_psnr=float(np.mean(cc_psnr)), std_cc_psnr=float(np.std(cc_psnr)), mean_cc_ssim=float(np.mean(cc_ssim)),
                   cc_transforms=m[:, 8:20].reshape(-1, 3, 4).tolist())
    if timed:
        res["mean_inference_time"] = float(np.mean(times))
    return res
