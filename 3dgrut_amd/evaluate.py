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

`pose_aligned={...}` additionally scores every view POSE-ALIGNED (pose_align.PoseAligner): after the view has been
scored at its given pose, its pose is optimised against its photo with the model frozen, and the render at the aligned pose is
scored next to the plain one, so that a run that refined its training poses is not charged for the held-out poses it never saw.
"""
import copy
import os

import numpy as np
import torch

from .losses import apply_exposure, image_metrics, image_metrics_colour_corrected
from .pose_align import DeviceStep, PoseAligner


def _check_batch(batch, what):
    if getattr(batch, "rgb_gt", None) is None:
        raise ValueError(f"{what}: every batch needs rgb_gt")


def _save_image(rgb, path):
    from PIL import Image
    Image.fromarray(rgb.mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy()).save(path)


def evaluate(model, tracer, batches, out_dir=None, step=0, colour_corrected=False, ridge=1e-6, pose_aligned=None):
    """Render and score `batches`.  A batch's mask is ignored: every metric is of the full image, as in the reference, whose
    render.py and validation metrics never read the mask (it enters the training losses only).  Returns dict(psnr=[...],
    ssim=[...], mse=[...], l1=[...], mean_psnr, std_psnr (population std, as np.std), mean_ssim, n_views) and, when the tracer was
    built with render.enable_kernel_timings, mean_inference_time (ms per frame, the mean of the library's forward_render times).
    out_dir: the renders are written to out_dir/ours_{step}/renders/{i:05d}.png (clamped and rounded as torchvision.utils.save_image
    does).
    colour_corrected: every view is also scored through its fitted colour transform (ridge: the fit's regulariser, > 0); the plain
    metrics are the same calls and the same bits, and the result gains cc_psnr, cc_ssim, cc_mse, cc_l1 (lists), mean_cc_psnr,
    std_cc_psnr, mean_cc_ssim and cc_transforms ([V][3][4], the fitted [A | b] per view); with out_dir the corrected renders go to
    out_dir/ours_{step}/renders_cc/{i:05d}.png.
    pose_aligned: None, or the aligner's settings as a dict (iterations, lr_translation in WORLD units, lr_rotation in radians, and
    optionally beta1, beta2, eps, lambda_l1, lambda_ssim; pose_align.DEFAULTS, UNTUNED on real captures).  Every view is first scored
    at its given pose exactly as without the option (the same calls, the same bits, the same timing sample), then aligned, rendered
    at the aligned pose through the same tracer.render and scored again.  The result gains pa_psnr, pa_ssim, pa_mse, pa_l1 (lists),
    mean_pa_psnr, std_pa_psnr, mean_pa_ssim, pa_poses ([V][4][4]), pa_translation, pa_rotation_deg (the aligned pose against the
    given one), pa_best_iteration, pa_loss_given, pa_loss_aligned (lists), mean_pa_translation, mean_pa_rotation_deg and, with
    colour_corrected, pa_cc_psnr, pa_cc_ssim, pa_cc_mse, pa_cc_l1, mean_pa_cc_psnr, std_pa_cc_psnr, mean_pa_cc_ssim; with out_dir the
    aligned renders go to out_dir/ours_{step}/renders_pa/{i:05d}.png.  A batch's mask enters the alignment loss and no score.  The
    model's tensors are never written."""
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
        if pose_aligned is not None:
            os.makedirs(os.path.join(out_dir, f"ours_{int(step)}", "renders_pa"), exist_ok=True)
    dev = batches[0].rays_ori.device
    metrics = torch.empty((len(batches), 4), dtype=torch.float32, device=dev)
    if colour_corrected:
        cc_metrics = torch.empty((len(batches), 4), dtype=torch.float32, device=dev)
        cc_transforms = torch.empty((len(batches), 12), dtype=torch.float32, device=dev)
    aligner, aligned = None, []
    if pose_aligned is not None:
        pa = dict(pose_aligned)
        # the frozen model's activated, packed rows: once per pass
        device_step = DeviceStep(model, tracer, lambda_l1=pa.pop("lambda_l1", 0.8), lambda_ssim=pa.pop("lambda_ssim", 0.2))
        pa.pop("enabled", None)
        pa.pop("validation", None)
        betas = (pa.pop("beta1", 0.9), pa.pop("beta2", 0.999))
        aligner = PoseAligner(device_step, betas=betas, **pa)
        pa_metrics = torch.empty((len(batches), 8 if colour_corrected else 4), dtype=torch.float32, device=dev)
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
            if aligner is not None:
                found = aligner.align(batch)
                aligned.append(found)
                at = copy.copy(batch)
                at.T_to_world = torch.as_tensor(found["pose"], dtype=torch.float32).reshape(1, 4, 4)
                out = tracer.render(model, at, train=False, frame_id=int(step))
                rgba = torch.cat([out["pred_rgb"][0], out["pred_opacity"][0]], dim=-1)
                image_metrics(rgba, batch.rgb_gt, background=0.0, out=pa_metrics[i, 0:4])
                if colour_corrected:
                    image_metrics_colour_corrected(rgba, batch.rgb_gt, background=0.0, ridge=ridge, out=pa_metrics[i, 4:8])
                if render_dir is not None:
                    _save_image(out["pred_rgb"][0], os.path.join(os.path.dirname(render_dir), "renders_pa", f"{i:05d}.png"))
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
    if aligner is not None:
        p = pa_metrics.cpu().double().numpy()
        col = lambda k: [a[k] for a in aligned]
        res.update(pa_psnr=p[:, 1].tolist(), pa_ssim=p[:, 2].tolist(), pa_mse=p[:, 0].tolist(), pa_l1=p[:, 3].tolist(),
                   mean_pa_psnr=float(np.mean(p[:, 1])), std_pa_psnr=float(np.std(p[:, 1])), mean_pa_ssim=float(np.mean(p[:, 2])),
                   pa_poses=[a["pose"].tolist() for a in aligned], pa_translation=col("translation"), pa_rotation_deg=col("rotation_deg"),
                   pa_best_iteration=col("best_iteration"), pa_loss_given=col("loss_given"), pa_loss_aligned=col("loss_aligned"),
                   mean_pa_translation=float(np.mean(col("translation"))), mean_pa_rotation_deg=float(np.mean(col("rotation_deg"))))
        if colour_corrected:
            res.update(pa_cc_psnr=p[:, 5].tolist(), pa_cc_ssim=p[:, 6].tolist(), pa_cc_mse=p[:, 4].tolist(), pa_cc_l1=p[:, 7].tolist(),
                       mean_pa_cc_psnr=float(np.mean(p[:, 5])), std_pa_cc_psnr=float(np.std(p[:, 5])), mean_pa_cc_ssim=float(np.mean(p[:, 6])))
    if timed:
        res["mean_inference_time"] = float(np.mean(times))
    return res
