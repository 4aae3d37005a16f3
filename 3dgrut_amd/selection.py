"""Selecting Gaussians from 2-D masks, and showing the selection in a view.

Over the label masks L_v (0/1, [H,W]) of the views that have one:

    share_i    = sum_v weighted_sum_i(L_v) / sum_v weight_sum_i      both sums from ContributionScores.accumulate(batch,
                 pixel_weight=L_v) over exactly those views, as q32 integers: the share does not depend on the order of the views
    selected_i = share_i > threshold and pixels_i >= min_pixels
    s(p)       = render(1{selected})(p), in [0, alpha(p)]            the rendered selection of a view (attributes.AttributeRenderer)
    predicted  = s(p) > 0.5                                          more than half of the pixel is drawn by selected Gaussians
    IoU        = |pred and L| / |pred or L|, 1.0 when both are empty

The lift is the weighted contribution walk, the rendering its other direction (gut_trace_attributes): a lift can
be checked by rendering it into a view it was not made from and comparing with that view's own mask.
"""
import numpy as np
import torch

from . import contribution
from .confblock import boolean, check_block, integer, nonempty_string, number


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def share_of(weighted_sum, weight_sum):
    """weighted_sum / weight_sum as float64, 0 where weight_sum is 0 (a Gaussian no view drew has no share); tensors or arrays."""
    if isinstance(weight_sum, torch.Tensor):
        ws, w = weighted_sum.to(torch.float64), weight_sum.to(torch.float64)
        return torch.where(w > 0, ws / torch.where(w > 0, w, torch.ones_like(w)), torch.zeros_like(w))
    ws, w = np.asarray(weighted_sum, np.float64), np.asarray(weight_sum, np.float64)
    return np.where(w > 0, ws / np.where(w > 0, w, 1.0), 0.0)


def lift_masks(model, tracer, batches, masks):
    """The label masks of the batches' views lifted to `model`'s rows: dict(share float64 [N], weight_sum float64 [N], pixels int64
    [N], n_views) on the model's device.  masks: one [H,W] tensor or array of 0 / 1 per batch (any shape with H * W elements)."""
    batches, masks = list(batches), list(masks)
    if len(batches) != len(masks):
        raise ValueError(f"lift_masks: {len(batches)} views and {len(masks)} masks")
    if not batches:
        raise ValueError("lift_masks: no view to lift from")
    scorer = contribution.ContributionScores(model, tracer)
    for batch, mask in zip(batches, masks):
        H, W = int(batch.rays_ori.shape[1]), int(batch.rays_ori.shape[2])
        plane = torch.as_tensor(mask).to(device=scorer.act.device, dtype=torch.float32)
        if plane.numel() != H * W:
            raise ValueError(f"lift_masks: a mask of {tuple(plane.shape)} for a view of {H}x{W}")
        scorer.accumulate(batch, pixel_weight=plane.reshape(H, W).contiguous())
    res = scorer.result()
    return dict(share=share_of(res["weighted_sum"], res["weight_sum"]), weight_sum=res["weight_sum"], pixels=res["pixels"],
                n_views=res["n_views"])


def select(lifted, threshold=0.5, min_pixels=1):
    """bool [N] like lifted["share"] (a tensor on its device, or numpy): share > threshold (strictly) and pixels >= min_pixels; a
    row without drawn weight is never selected."""
    t = float(threshold)
    if isinstance(threshold, (bool, str)) or not (0.0 <= t <= 1.0):
        raise ValueError(f"threshold must be in [0, 1], got {threshold!r}")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or int(min_pixels) < 0:
        raise ValueError(f"min_pixels must be an integer >= 0, got {min_pixels!r}")
    return (lifted["share"] > t) & (lifted["pixels"] >= int(min_pixels)) & (lifted["weight_sum"] > 0)


def render_selection(renderer, batch, selected):
    """s(p): the selection bool [N] rendered into the batch's view by an attributes.AttributeRenderer, float32 [H,W]."""
    return renderer.render(batch, torch.as_tensor(selected))[0]


def mask_iou(pred, label):
    """|pred and label| / |pred or label| of two boolean masks of one shape; 1.0 when both are empty."""
    p, l = _host(pred).astype(bool), _host(label).astype(bool)
    if p.shape != l.shape:
        raise ValueError(f"mask_iou: shapes {p.shape} and {l.shape}")
    union = int((p | l).sum())
    return 1.0 if union == 0 else int((p & l).sum()) / union


def split_rows(stepper_or_model, selected):
    """(rows selected, the other rows): int64 index tensors on the model's device, each in row order — what compaction's row
    subsetting (strategy._StateOps.keep) selects with; io_ply.export_native_model(model, path, rows=...) writes either part."""
    model = getattr(stepper_or_model, "model", stepper_or_model)
    n = int(model.raw.shape[0])
    mask = torch.as_tensor(selected, dtype=torch.bool, device=model.raw.device)
    if tuple(mask.shape) != (n,):
        raise ValueError(f"split_rows: the selection must be [{n}], got {tuple(mask.shape)}")
    return mask.nonzero().squeeze(1), (~mask).nonzero().squeeze(1)


# the trainer's `selection` block
DEFAULTS = {"enabled": False, "mask_suffix": "_object", "threshold": 0.5, "min_pixels": 1}
RULES = {"enabled": boolean(), "mask_suffix": nonempty_string(), "threshold": number("in [0, 1]", ge=0, le=1), "min_pixels": integer(ge=0)}


def check_config(block):
    """The resolved `selection` block: enabled true or false, mask_suffix a non-empty string, threshold in [0, 1], min_pixels an
    integer >= 0."""
    return check_block("selection", block, DEFAULTS, RULES)
