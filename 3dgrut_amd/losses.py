"""Loss functions of the train step (reference: threedgrut/model/losses.py, trainer.py:387-450).

`fused_ssim(img1, img2, padding="valid")` has the call signature of the external CUDA package the reference
imports; here it runs the HIP kernels of csrc/gut_ssim.hip through the C ABI.  img: [B,C,H,W] (any strides:
the permuted view of the tracer's [B,H,W,3] output is consumed in place); only img1 is differentiable.
"""
import ctypes as C

import torch

from . import _capi


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        if img1.dim() != 4 or img1.shape != img2.shape:
            raise RuntimeError("[fused_ssim] expected two [B,C,H,W] tensors of equal shape")
        if not img1.is_cuda or img1.dtype != torch.float32 or img2.dtype != torch.float32:
            raise RuntimeError("[fused_ssim] expected float32 GPU tensors (there is no CPU path)")
        lib = _capi.load()
        B, Cn, H, W = img1.shape
        img2 = img2.detach()
        if img2.stride() != img1.stride():
            img2 = _match_strides(img2, img1)
        ws_bytes = lib.gut_ssim_workspace_bytes(Cn, H, W)
        ws = torch.empty((B, (ws_bytes + 3) // 4), dtype=torch.float32, device=img1.device)
        out = torch.empty((B,), dtype=torch.float32, device=img1.device)
        stream = torch.cuda.current_stream(img1.device).cuda_stream
        sb, sc, sh, sw = img1.stride()
        with torch.cuda.device(img1.device):
            for b in range(B):
                rc = lib.gut_ssim_forward(C.c_void_p(stream), Cn, H, W, sc, sh, sw, img1.data_ptr() + 4 * b * sb,
                                          img2.data_ptr() + 4 * b * sb, ws[b].data_ptr(), out[b:].data_ptr())
                if rc:
                    raise RuntimeError(f"[fused_ssim] forward failed ({rc}); images must exceed 10x10")
        ctx.save_for_backward(img1, img2, ws)
        return out.mean()

    @staticmethod
    def backward(ctx, grad_out):
        img1, img2, ws = ctx.saved_tensors
        lib = _capi.load()
        B, Cn, H, W = img1.shape
        grad = torch.empty_strided(img1.shape, img1.stride(), dtype=torch.float32, device=img1.device)
        up = (grad_out.reshape(1).to(torch.float32) / B).contiguous()
        stream = torch.cuda.current_stream(img1.device).cuda_stream
        sb, sc, sh, sw = img1.stride()
        with torch.cuda.device(img1.device):
            for b in range(B):
                rc = lib.gut_ssim_backward(C.c_void_p(stream), Cn, H, W, sc, sh, sw, img1.data_ptr() + 4 * b * sb,
                                           img2.data_ptr() + 4 * b * sb, ws[b].data_ptr(), up.data_ptr(),
                                           grad.data_ptr() + 4 * b * sb)
                if rc:
                    raise RuntimeError(f"[fused_ssim] backward failed ({rc})")
        return grad, None


def _match_strides(src, like):
    out = torch.empty_strided(like.shape, like.stride(), dtype=src.dtype, device=src.device)
    out.copy_(src)
    return out


def fused_ssim(img1, img2, padding="valid", train=True):
    if padding != "valid":
        raise RuntimeError('[fused_ssim] only padding="valid" (the reference\'s setting) is built')
    return _FusedSSIM.apply(img1, img2)


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def regularisation_loss(density, scale, lambda_opacity, lambda_scale):
    """The MCMC recipe's regularisers (trainer.py:432-446): (lambda_opacity * mean |density|, lambda_scale * mean |scale|) for the
    ACTIVATED density [N,1] and scale [N,3] (model.get_density() / get_scale()); the means run over N and 3N values."""
    return lambda_opacity * density.abs().mean(), lambda_scale * scale.abs().mean()


def loss_weights(loss_conf):
    """The reference's `loss:` block (configs/base_gs.yaml:111-126, base_mcmc.yaml:13-18; a plain dict) -> the trainers' keyword
    arguments dict(lambda_l1, lambda_ssim, lambda_opacity, lambda_scale), a term whose `use_*` switch is off (or absent) weighted 0
    (trainer.py:406-447).  As in the reference, `use_l2` / `lambda_l2` do not enter the total loss: trainer.py:449 computes the L2 term
    and sums only L1, SSIM, opacity and scale — so they are ignored here."""
    def weight(name):
        return float(loss_conf.get(f"lambda_{name}", 0.0)) if loss_conf.get(f"use_{name}", False) else 0.0
    return dict(lambda_l1=weight("l1"), lambda_ssim=weight("ssim"), lambda_opacity=weight("opacity"), lambda_scale=weight("scale"))


def _constant_background(background, who, forms="'black', 'white' or a number"):
    """A constant background given as "black", "white" or a number, as the number."""
    bg = {"black": 0.0, "white": 1.0}.get(background, background)
    if isinstance(bg, str):
        raise ValueError(f"{who}: background must be {forms}, got {background!r}")
    return bg


def _view_images(rgba, gt_rgb, who):
    """The images of one view as every GPU entry point here takes them: a leading 1 squeezed, rgba [H,W,4] against gt_rgb [H,W,3],
    both float32 on one GPU."""
    rgba = rgba.reshape(rgba.shape[-3:]) if rgba.dim() == 4 and rgba.shape[0] == 1 else rgba
    gt_rgb = gt_rgb.reshape(gt_rgb.shape[-3:]) if gt_rgb.dim() == 4 and gt_rgb.shape[0] == 1 else gt_rgb
    if rgba.dim() != 3 or rgba.shape[2] != 4 or tuple(gt_rgb.shape) != (rgba.shape[0], rgba.shape[1], 3):
        raise RuntimeError(f"[{who}] expected rgba [H,W,4] and gt [H,W,3], got {tuple(rgba.shape)} and {tuple(gt_rgb.shape)}")
    if not rgba.is_cuda or rgba.dtype != torch.float32 or gt_rgb.dtype != torch.float32 or gt_rgb.device != rgba.device:
        raise RuntimeError(f"[{who}] expected float32 GPU tensors on one device (there is no CPU path)")
    return rgba, gt_rgb


def image_metrics(rgba, gt_rgb, background="black", out=None):
    """Evaluation metrics of one view on the GPU (gut_image_metrics, csrc/gut_ssim.hip): a float32 device tensor [4] = (MSE, PSNR,
    SSIM, L1) of image = rgb + background * (1 - alpha) against gt_rgb, unclamped, as the reference scores outputs["pred_rgb"]
    (render.py:137-285; PSNR for a data range of 1, SSIM the valid-region mean of the training loss).  rgba: [H,W,4] (or [1,H,W,4]),
    gt_rgb: [H,W,3] (or [1,H,W,3]), both float32 on the GPU; background: "black", "white" or 0.0 / 1.0.  out: a float32 device
    tensor of 4 contiguous elements to write into (e.g. row i of an evaluation pass's [V,4] tensor); nothing is read back."""
    bg = _constant_background(background, "image_metrics")
    rgba, gt_rgb = _view_images(rgba, gt_rgb, "image_metrics")
    rgba, gt_rgb = rgba.contiguous(), gt_rgb.contiguous()
    if out is None:
        out = torch.empty((4,), dtype=torch.float32, device=rgba.device)
    elif out.dtype != torch.float32 or out.device != rgba.device or out.numel() != 4 or not out.is_contiguous():
        raise RuntimeError("[image_metrics] out must be a contiguous float32 tensor of 4 elements on the images' device")
    lib = _capi.load()
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    ws = torch.empty(((lib.gut_image_metrics_workspace_bytes(H, W) + 3) // 4,), dtype=torch.float32, device=rgba.device)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = lib.gut_image_metrics(C.c_void_p(stream), H, W, rgba.data_ptr(), gt_rgb.data_ptr(), float(bg), ws.data_ptr(), out.data_ptr())
    if rc:
        raise RuntimeError(f"[image_metrics] failed ({rc}); images must exceed 10x10")
    return out


def colour_correction(comp, gt_rgb, ridge=1e-6):
    """The affine colour transform that fits an image best to its photo, in float64 torch on the tensors' device: the
    documented restatement of what gut_image_metrics_cc fits, for host tensors and tests.  comp [...,3] (the image composited over its
    background) and gt_rgb of the same shape; with x = (comp, 1) per pixel and P pixels, E = [A | b] minimises
        sum |A comp + b - gt|^2 + ridge * P * |[A | b] - [I | 0]|_F^2,
    i.e. G = sum x x^T + ridge P I_4, C = sum x gt^T + ridge P [I_3; 0], E^T = G^-1 C.  ridge > 0 belongs to the definition: G is
    positive definite whatever the image, and what the data do not show stays at the identity.  Returns E [3,4] float64."""
    ridge = float(ridge)
    if not (0.0 < ridge < float("inf")):
        raise ValueError(f"colour_correction: ridge must be finite and > 0, got {ridge!r}")
    if comp.shape[-1] != 3 or tuple(gt_rgb.shape) != tuple(comp.shape):
        raise ValueError(f"colour_correction: expected two [...,3] tensors of one shape, got {tuple(comp.shape)} and {tuple(gt_rgb.shape)}")
    x = comp.detach().reshape(-1, 3).to(torch.float64)
    y = gt_rgb.detach().reshape(-1, 3).to(device=x.device, dtype=torch.float64)
    x = torch.cat([x, torch.ones((x.shape[0], 1), dtype=torch.float64, device=x.device)], dim=1)
    eye = torch.eye(4, dtype=torch.float64, device=x.device)
    rp = ridge * x.shape[0]
    G = x.transpose(0, 1) @ x + rp * eye
    Cm = x.transpose(0, 1) @ y + rp * eye[:, :3]
    return torch.cholesky_solve(Cm, torch.linalg.cholesky(G)).transpose(0, 1).contiguous()


def image_metrics_colour_corrected(rgba, gt_rgb, background="black", ridge=1e-6, out=None, exposure_out=None):
    """Colour-corrected evaluation metrics of one view on the GPU (gut_image_metrics_cc, csrc/gut_ssim.hip): the
    affine E of colour_correction is fitted to image = rgb + background * (1 - alpha) against gt_rgb on the device (moments and solve
    in double), and (MSE, PSNR, SSIM, L1) are those of E [image; 1], unclamped, with image_metrics' counts.  Arguments as
    image_metrics; ridge: finite and > 0.  out: a contiguous float32 device tensor of 4 elements to write into; exposure_out: one of
    12 (a [12] or [3,4] tensor, e.g. row i of an evaluation pass's [V,12]) that receives E.  Returns (out, E [3,4]), both on the
    device; nothing is read back."""
    bg = _constant_background(background, "image_metrics_colour_corrected")
    ridge = float(ridge)
    if not (0.0 < ridge < float("inf")):
        raise ValueError(f"image_metrics_colour_corrected: ridge must be finite and > 0, got {ridge!r}")
    rgba, gt_rgb = _view_images(rgba, gt_rgb, "image_metrics_colour_corrected")
    rgba, gt_rgb = rgba.contiguous(), gt_rgb.contiguous()
    if out is None:
        out = torch.empty((4,), dtype=torch.float32, device=rgba.device)
    elif out.dtype != torch.float32 or out.device != rgba.device or out.numel() != 4 or not out.is_contiguous():
        raise RuntimeError("[image_metrics_colour_corrected] out must be a contiguous float32 tensor of 4 elements on the images' device")
    if exposure_out is None:
        exposure_out = torch.empty((3, 4), dtype=torch.float32, device=rgba.device)
    elif exposure_out.dtype != torch.float32 or exposure_out.device != rgba.device or tuple(exposure_out.shape) not in ((12,), (3, 4)) \
            or not exposure_out.is_contiguous():
        raise RuntimeError("[image_metrics_colour_corrected] exposure_out must be a contiguous float32 [12] or [3,4] tensor on the "
                           "images' device")
    lib = _capi.load()
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    # (float64 elements: the rows of moments in the workspace are doubles, and the allocation is aligned for them)
    ws = torch.empty(((lib.gut_image_metrics_cc_workspace_bytes(H, W) + 7) // 8,), dtype=torch.float64, device=rgba.device)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = lib.gut_image_metrics_cc(C.c_void_p(stream), H, W, rgba.data_ptr(), gt_rgb.data_ptr(), float(bg), ridge, ws.data_ptr(),
                                      out.data_ptr(), exposure_out.data_ptr())
    if rc:
        raise RuntimeError(f"[image_metrics_colour_corrected] failed ({rc})" + ("; images must exceed 10x10" if rc == 1 else ""))
    return out, exposure_out.reshape(3, 4)


def apply_exposure(pred_rgb, exposure):
    """The affine image of a view: pred_rgb [...,3] (composited over its background) -> A pred + b per pixel, with
    exposure = [A | b] given as [3,4] or [12] (row-major), of pred_rgb's dtype and device; differentiable in both."""
    E = exposure.reshape(3, 4)
    return pred_rgb @ E[:, :3].transpose(0, 1) + E[:, 3]


def bilateral_slice(comp, grid):
    """The bilateral slice of a view, the definition in plain differentiable torch: comp [H,W,3] or [1,H,W,3] (the
    image composited over its background), grid [12,L,Gh,Gw] of comp's dtype and device -> the image of comp's shape, every pixel
    through the 3x4 transform the grid holds at (x, y, luminance), trilinear with corners aligned.  Differentiable in both; the
    guidance is differentiated (inside 0 < g < 1: at a level boundary the derivative of the piece the pixel lies in, outside 0)."""
    if comp.shape[-1] != 3 or comp.dim() not in (3, 4) or (comp.dim() == 4 and comp.shape[0] != 1):
        raise ValueError(f"bilateral_slice: comp must be [H,W,3] or [1,H,W,3], got {tuple(comp.shape)}")
    if grid.dim() != 4 or grid.shape[0] != 12:
        raise ValueError(f"bilateral_slice: grid must be [12,L,Gh,Gw], got {tuple(grid.shape)}")
    H, W = int(comp.shape[-3]), int(comp.shape[-2])
    L, Gh, Gw = (int(n) for n in grid.shape[1:])
    c = comp.reshape(H, W, 3)
    dt, dev = c.dtype, c.device
    g = (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]
    inside = (g > 0) & (g < 1)
    gc = torch.where(inside, g, torch.nan_to_num(g.detach(), nan=0.0).clamp(0.0, 1.0))   # the gradient passes inside only

    def axis(s, n):
        i0 = torch.floor(s.detach())
        f = s - i0
        i0 = i0.long().clamp(0, n - 1)
        return f, i0, (i0 + 1).clamp(max=n - 1)

    sx = torch.arange(W, dtype=dt, device=dev) * ((Gw - 1) / (W - 1) if W > 1 else 0.0)
    sy = torch.arange(H, dtype=dt, device=dev) * ((Gh - 1) / (H - 1) if H > 1 else 0.0)
    fx, c0, c1 = axis(sx[None, :].expand(H, W), Gw)
    fy, r0, r1 = axis(sy[:, None].expand(H, W), Gh)
    fz, z0, z1 = axis(gc * (L - 1), L)
    A = None
    for z, wz in ((z0, 1 - fz), (z1, fz)):
        for r, wy in ((r0, 1 - fy), (r1, fy)):
            for col, wx in ((c0, 1 - fx), (c1, fx)):
                term = ((wx * wy) * wz)[None] * grid[:, z, r, col]           # [12,H,W]
                A = term if A is None else A + term
    A = A.reshape(3, 4, H, W)
    out = ((A[:, 0] * c[..., 0] + A[:, 1] * c[..., 1]) + A[:, 2] * c[..., 2]) + A[:, 3]   # [3,H,W]
    return out.permute(1, 2, 0).reshape(comp.shape)


def bilateral_total_variation(grid):
    """TV(G) of DESIGN.md §21 for grid [...,12,L,Gh,Gw]: per axis the mean of the squared differences of adjacent cells (over the
    pairs and the 12 channels), summed over the axes; an axis of length 1 adds 0.  Differentiable; [...] out."""
    tv = grid.new_zeros(grid.shape[:-4])
    for dim in (-1, -2, -3):
        if grid.shape[dim] > 1:
            d = grid.narrow(dim, 1, grid.shape[dim] - 1) - grid.narrow(dim, 0, grid.shape[dim] - 1)
            tv = tv + (d * d).mean(dim=(-4, -3, -2, -1))
    return tv


def photometric_loss(pred_rgb, gt_rgb, lambda_l1=0.8, lambda_ssim=0.2, mask=None, exposure=None):
    """pred/gt [B,H,W,3].  lambda_l1*L1 + lambda_ssim*(1-SSIM)  (configs/base_gs.yaml:111-119, trainer.py:425-449).
    mask [B,H,W,1] (Batch.mask) or None: both images are multiplied by it first, as the reference's get_losses does
    (trainer.py:397-404); the means keep their full-image counts.
    exposure [3,4] / [12] or None: the prediction is passed through apply_exposure first (before the mask).
    float32 GPU tensors go through the HIP SSIM (fused_ssim); host or fp64 tensors through train.ssim, the same definition in torch."""
    if exposure is not None:
        pred_rgb = apply_exposure(pred_rgb, exposure)
    if mask is not None:
        mask = mask.to(device=pred_rgb.device, dtype=pred_rgb.dtype)
        pred_rgb, gt_rgb = pred_rgb * mask, gt_rgb * mask
    if pred_rgb.is_cuda and pred_rgb.dtype == torch.float32:
        s = fused_ssim(pred_rgb.permute(0, 3, 1, 2), gt_rgb.permute(0, 3, 1, 2), padding="valid")
    else:
        # host or fp64 tensors (the tests' references): the same SSIM in plain torch, in the tensors' own precision
        from .train import ssim
        s = ssim(pred_rgb.permute(0, 3, 1, 2), gt_rgb.to(pred_rgb.dtype).permute(0, 3, 1, 2))
    return lambda_l1 * l1_loss(pred_rgb, gt_rgb) + lambda_ssim * (1.0 - s)


def _plane_mask(mask, H, W, device):
    """A mask given as [H,W], [H,W,1] or [1,H,W,1] (Batch.mask of one view; any dtype) as contiguous float32 [H,W] on `device`."""
    shape = tuple(mask.shape)
    if shape not in ((H, W), (H, W, 1), (1, H, W, 1)):
        raise ValueError(f"fused_photometric_loss: mask must be [{H},{W}], [{H},{W},1] or [1,{H},{W},1] for these images, "
                         f"got {shape}")
    return mask.reshape(H, W).to(device=device, dtype=torch.float32).contiguous()


def _plane_background(background, H, W, device):
    """A background tensor given as [H,W,3], [1,H,W,3] or [3] (one RGB colour, expanded here; any dtype or device) as contiguous
    float32 [H,W,3] on `device`."""
    shape = tuple(background.shape)
    if shape == (3,):
        background = background.reshape(1, 1, 3).expand(H, W, 3)
    elif shape not in ((H, W, 3), (1, H, W, 3)):
        raise ValueError(f"fused_photometric_loss: a background tensor must be [{H},{W},3], [1,{H},{W},3] or [3] for these images, "
                         f"got {shape}")
    return background.reshape(H, W, 3).to(device=device, dtype=torch.float32).contiguous()


def _exposure12(exposure, device):
    """An exposure given as a float32 [12] or [3,4] tensor on `device`, as contiguous [12] (a view where it already is)."""
    if not isinstance(exposure, torch.Tensor) or tuple(exposure.shape) not in ((12,), (3, 4)):
        raise ValueError(f"fused_photometric_loss: exposure must be a [12] or [3,4] tensor, got "
                         f"{tuple(exposure.shape) if isinstance(exposure, torch.Tensor) else type(exposure).__name__}")
    if exposure.dtype != torch.float32 or exposure.device != device:
        raise ValueError(f"fused_photometric_loss: exposure must be float32 on {device} (the kernels read it there), got "
                         f"{exposure.dtype} on {exposure.device}")
    return exposure.detach().reshape(12).contiguous()


def fused_photometric_loss(rgba, gt_rgb, background, lambda_l1=0.8, lambda_ssim=0.2, mask=None, workspace=None, exposure=None,
                           exposure_grad=True):
    """The train step's loss and its gradient without autograd (gut_photometric_loss_run, csrc/gut_ssim.hip):
    loss = lambda_l1 * L1 + lambda_ssim * (1 - SSIM) of image = mask * (A (rgb + B * (1 - alpha)) + b) against mask * gt_rgb.
    rgba [H,W,4] (or [1,H,W,4]) and gt_rgb [H,W,3] (or [1,H,W,3]): contiguous float32 on one GPU.  The operands:
    background (B): "black", "white" or 0.0 / 1.0, or a tensor of any dtype or device — [H,W,3] / [1,H,W,3], every pixel over its own
    colour (the reference's `random` background, model/background.py:83-89, or an environment image), or [3], one RGB colour.
    mask: None, or [H,W] / [H,W,1] / [1,H,W,1] of any dtype (trainer.py:397-404); the means keep their full-image counts, and a
    pixel whose mask is 0 gets a gradient of exactly zero.
    exposure: None, or the view's affine colour transform E = [A | b] as a float32 [12] / [3,4] tensor on the images' device
    (DESIGN.md §10), applied before the mask.
    workspace: a float32 device tensor to reuse, or None: at least gut_photometric_workspace_bytes(H, W) bytes, with an exposure
    gut_photometric_exposure_workspace_bytes(H, W).
    Returns (loss3, rgba_grad): a float32 device tensor (loss, L1, SSIM) and d(loss)/d(rgba) [H,W,4]; with an exposure (loss3,
    rgba_grad, exposure_grad12), d(loss)/dE laid out like E — None with exposure_grad=False, which applies E and reduces nothing."""
    plane = isinstance(background, torch.Tensor)
    bg = background if plane else _constant_background(background, "fused_photometric_loss", "'black', 'white', a number or a tensor")
    rgba, gt_rgb = _view_images(rgba, gt_rgb, "fused_photometric_loss")
    if not rgba.is_contiguous() or not gt_rgb.is_contiguous():
        raise RuntimeError("[fused_photometric_loss] expected contiguous tensors")
    lib = _capi.load()
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if mask is not None:
        mask = _plane_mask(mask, H, W, rgba.device)
    bg = _plane_background(bg, H, W, rgba.device) if plane else float(bg)
    if exposure is not None:
        exposure = _exposure12(exposure, rgba.device)
    need = lib.gut_photometric_workspace_bytes(H, W) if exposure is None else lib.gut_photometric_exposure_workspace_bytes(H, W)
    if workspace is None:
        workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=rgba.device)
    elif workspace.dtype != torch.float32 or workspace.device != rgba.device or workspace.numel() * 4 < need or not workspace.is_contiguous():
        raise RuntimeError(f"[fused_photometric_loss] workspace must be a contiguous float32 tensor of at least {need} bytes on the images' device")
    with torch.cuda.device(rgba.device):
        if exposure is not None:
            grad12 = torch.empty((12,), dtype=torch.float32, device=rgba.device) if exposure_grad else None
            return (*_photometric_loss_call(lib, H, W, rgba, gt_rgb, bg, lambda_l1, lambda_ssim, mask, workspace, exposure, grad12), grad12)
        return _photometric_loss_call(lib, H, W, rgba, gt_rgb, bg, lambda_l1, lambda_ssim, mask, workspace)


def _photometric_loss_call(lib, H, W, rgba, gt_rgb, bg, lambda_l1, lambda_ssim, mask, workspace, exposure=None, exposure_grad=None):
    """The one C call behind fused_photometric_loss (gut_photometric_loss_run), nothing checked: contiguous float32 device tensors
    (gt_rgb with or without a leading 1), the images' device current.  NativeTrainStep calls this directly every step, on buffers
    it sized itself.  The operands: bg a float or a float32 [H,W,3] device plane; mask a float32 [H,W] plane or None; exposure a
    contiguous float32 [12] device tensor or None, and exposure_grad the [12] device tensor that receives d(loss)/dE, or None.
    workspace: gut_photometric_workspace_bytes(H, W), with an exposure gut_photometric_exposure_workspace_bytes(H, W)."""
    # three fresh floats every call (the caching allocator, no kernel): callers return views of them
    loss3 = torch.empty((3,), dtype=torch.float32, device=rgba.device)
    rgba_grad = torch.empty_like(rgba)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    plane = isinstance(bg, torch.Tensor)
    ptr = lambda t: None if t is None else t.data_ptr()
    desc = _capi.GutPhotometricLoss(rgba.data_ptr(), gt_rgb.data_ptr(), ptr(mask), bg.data_ptr() if plane else None, ptr(exposure),
                                    workspace.data_ptr(), loss3.data_ptr(), rgba_grad.data_ptr(), ptr(exposure_grad),
                                    0.0 if plane else bg, lambda_l1, lambda_ssim)
    rc = lib.gut_photometric_loss_run(C.c_void_p(stream), H, W, C.byref(desc))
    if rc:
        raise RuntimeError(f"[3dgut] photometric_loss failed ({rc}): " + ("a null pointer, or an image of 10x10 pixels or less"
                                                                         if rc == 1 else "the kernel launch failed"))
    return loss3, rgba_grad


def pixel_error(rgba, gt_rgb, background=0.0, mask=None, exposure=None):
    """The per-pixel rendering error of a view, in float64 torch on rgba's device: the definition that
    fused_pixel_error (gut_pixel_error) computes in float32, for host tensors and tests.
        comp = rgb + B (1 - alpha),  img = A comp + b with exposure E = [A | b] (comp without),
        error = clamp(mean over the three channels of |img - gt|, 0, 1) * mask
    rgba [H,W,4], gt_rgb [H,W,3]; background: "black", "white", a number, or a tensor that broadcasts to [H,W,3]; mask None or
    [H,W] / [H,W,1]; exposure None or [3,4] / [12].  Returns [H,W] float64."""
    f64 = lambda t: t.detach().to(device=rgba.device, dtype=torch.float64)
    B = f64(background) if isinstance(background, torch.Tensor) else float(_constant_background(background, "pixel_error"))
    x = f64(rgba)
    img = x[..., :3] + B * (1.0 - x[..., 3:4])
    if exposure is not None:
        img = apply_exposure(img, f64(exposure))
    e = (img - f64(gt_rgb)).abs().sum(-1).div(3.0).clamp(0.0, 1.0)
    return e if mask is None else e * f64(mask).reshape(e.shape)


def fused_pixel_error(rgba, gt_rgb, background, mask=None, exposure=None, out=None):
    """pixel_error on the GPU in one elementwise launch (gut_pixel_error, csrc/gut_ssim.hip): a float32 [H,W] plane in [0, 1], the
    weight plane of SplatRaster.trace_contribution for error-based densification.  The operands are fused_photometric_loss's: rgba
    [H,W,4] (or [1,H,W,4]) and gt_rgb [H,W,3] (or [1,H,W,3]) contiguous float32 on one GPU; background "black", "white", a number
    or a tensor ([H,W,3] / [1,H,W,3] / [3]); mask None or [H,W] / [H,W,1] / [1,H,W,1]; exposure None or a float32 [12] / [3,4]
    tensor on the images' device, read there.  out: a contiguous float32 [H,W] tensor on the device to write into.  Nothing is read back."""
    plane = isinstance(background, torch.Tensor)
    bg = background if plane else _constant_background(background, "fused_pixel_error", "'black', 'white', a number or a tensor")
    rgba, gt_rgb = _view_images(rgba, gt_rgb, "fused_pixel_error")
    if not rgba.is_contiguous() or not gt_rgb.is_contiguous():
        raise RuntimeError("[fused_pixel_error] expected contiguous tensors")
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if mask is not None:
        mask = _plane_mask(mask, H, W, rgba.device)
    bg = _plane_background(bg, H, W, rgba.device) if plane else float(bg)
    if exposure is not None:
        exposure = _exposure12(exposure, rgba.device)
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=rgba.device)
    elif out.dtype != torch.float32 or out.device != rgba.device or tuple(out.shape) != (H, W) or not out.is_contiguous():
        raise RuntimeError(f"[fused_pixel_error] out must be a contiguous float32 [{H},{W}] tensor on the images' device")
    ptr = lambda t: None if t is None else t.data_ptr()
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = _capi.load().gut_pixel_error(C.c_void_p(stream), H, W, rgba.data_ptr(), gt_rgb.data_ptr(), ptr(mask),
                                          bg.data_ptr() if plane else None, 0.0 if plane else bg, ptr(exposure), out.data_ptr())
    if rc:
        raise RuntimeError(f"[3dgut] pixel_error failed ({rc}): " + ("a null pointer" if rc == 1 else "the kernel launch failed"))
    return out
