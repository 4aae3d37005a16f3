"""Per-Gaussian contribution scores over a set of views, and compaction of a trained model by them.

The score of a Gaussian is built from the blending weights w = T * alpha the forward compositor forms for it (T: the ray's
transmittance in front of it) in every pixel in which it is composited, over the views it is accumulated over:

    weight_sum   the sum of w       (how much of the rendered images is this Gaussian's)
    max_weight   the largest w      (LightGaussian-style: a Gaussian that dominates a single pixel survives)
    pixels       the number of (view, pixel) pairs with w > 0

`ContributionScores` accumulates them on the GPU with the model frozen: a forward (SplatRaster.trace on rows activated and packed
ONCE per pass, as pose_align.DeviceStep does) and SplatRaster.trace_contribution (gut_trace_contribution) per view, no host
synchronisation in between.  The records are integers (the sum in units of 2^-32, the maximum as float bits, a count), updated by
integer atomics: the result is the same bit for bit whatever the order of the views, from run to run.

With a per-pixel plane e in [0, 1] (accumulate(batch, pixel_weight=plane)) the same walk also sums w * e:

    weighted_sum the sum of w * e   ("how much of the per-pixel quantity e did this Gaussian draw")

With e the rendering error of the view (accumulate_error) it is the error the Gaussian is responsible for, the score of error-based
densification (strategy.select_by_error).  With e a 2-D segmentation mask (0 or 1) it lifts the mask to the Gaussians:
weighted_sum / weight_sum is the share of the Gaussian's drawn weight that lies inside the mask, 1 for a Gaussian seen only inside
it, 0 for one seen only outside, over as many views as were accumulated; threshold it for a 3-D selection.

`keep_mask` turns a result into the rows to keep ("the best fraction"), deterministically; `compact` removes the others from a
NativeTrainStep's model together with their optimiser state, the way the densification strategies prune.
"""
import math

import numpy as np
import torch

from .confblock import boolean, check_block, integer, number, one_of

SCORES =("weight_sum", "max_weight")


def unpack_scores(scores):
    """The GutContribution records [N,2] int64 -> (weight_sum float64 [N], max_weight float32 [N], pixels int64 [N])."""
    words = scores.contiguous().view(torch.int32).reshape(-1, 4)
    weight_sum = scores[:, 0].to(torch.float64) * (2.0 ** -32)    # below 2^63: non-negative as int64
    max_weight = words[:, 2].contiguous().view(torch.float32)
    pixels = words[:, 3].to(torch.int64) & 0xFFFFFFFF
    return weight_sum, max_weight, pixels


class FrozenModel:
    """`model`'s rows as the rasteriser reads them, prepared once: the [N,12] activated rows, the [N,48] features, the number of
    active features, and the tracer's rasteriser.  forward(batch) renders a view from them and returns the forward's outputs with
    what a following call on the handle needs.  The model must not change while the object is in use."""

    def __init__(self, model, tracer):
        from .tracer import Tracer
        self._create_camera = Tracer.create_camera_parameters
        self.raster = tracer.tracer_wrapper
        with torch.no_grad():
            z = torch.zeros_like(model.get_density())
            self.act = torch.cat([model.positions, model.get_density(), model.get_rotation(), model.get_scale(), z], dim=1).to(torch.float32).contiguous()
            self.features = model.get_features().detach().to(torch.float32).contiguous()
        self.n_active_features = int(model.n_active_features)
        self.n_forwards = 0      # forwards rendered so far: what a later call that must follow ITS forward compares (attributes.py)

    def forward(self, batch):
        """(outs, rays_o, rays_d, cam): the forward's four outputs, the rays and the camera tail of the following call."""
        self.n_forwards += 1
        sensor, poses = self._create_camera(batch)
        rays_o, rays_d = batch.rays_ori.contiguous(), batch.rays_dir.contiguous()
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        outs = self.raster.trace(0, self.n_active_features, self.act, self.features, rays_o, rays_d, None, *cam)
        return outs, rays_o, rays_d, cam


class ContributionScores(FrozenModel):
    """Scores of `model`'s rows over the views handed to accumulate().  The [N,12] activated rows and the [N,48] features are
    prepared here, once; the model must not change while a pass runs."""

    def __init__(self, model, tracer):
        super().__init__(model, tracer)
        self.scores = torch.zeros((self.act.shape[0], 2), dtype=torch.int64, device=self.act.device)
        self.weighted = None     # uint64 [N] in units of 2^-32, held as int64 (torch has no uint64 arithmetic); created by the first plane
        self.n_views = 0

    def _accumulate(self, batch, plane_of):
        outs, rays_o, rays_d, cam = self.forward(batch)
        plane = plane_of(outs[0])
        if plane is None:
            self.raster.trace_contribution(0, self.n_active_features, self.act, rays_o, rays_d, *cam, self.scores)
        else:
            if self.weighted is None:
                self.weighted = torch.zeros((self.act.shape[0],), dtype=torch.int64, device=self.act.device)
            self.raster.trace_contribution(0, self.n_active_features, self.act, rays_o, rays_d, *cam, self.scores,
                                           pixel_weight=plane, weighted=self.weighted)
        self.n_views += 1
        return self

    def accumulate(self, batch, pixel_weight=None):
        """One forward at the batch's pose and its contribution walk; nothing is read back.  pixel_weight: a contiguous float32
        [H,W] plane on the device (clamped to [0, 1] by the kernel); the walk then also adds the sums of w * plane to weighted_sum."""
        return self._accumulate(batch, lambda rgba: pixel_weight)

    def accumulate_error(self, batch, background, mask=None, exposure=None):
        """accumulate() with the view's rendering error as the plane (losses.fused_pixel_error of the forward's image against
        batch.rgb_gt): the operands are fused_photometric_loss's — background "black", "white", a number or a tensor; mask None or
        the view's mask; exposure None or the view's float32 [12] / [3,4] device tensor."""
        from .losses import fused_pixel_error
        return self._accumulate(batch, lambda rgba: fused_pixel_error(rgba, batch.rgb_gt.contiguous(), background, mask=mask, exposure=exposure))

    def result(self):
        """dict(weight_sum float64 [N], max_weight float32 [N], pixels int64 [N], n_views), on the model's device; once a view was
        accumulated with a plane also weighted_sum float64 [N]."""
        weight_sum, max_weight, pixels = unpack_scores(self.scores)
        out = dict(weight_sum=weight_sum, max_weight=max_weight, pixels=pixels, n_views=self.n_views)
        if self.weighted is not None:
            out["weighted_sum"] = self.weighted.to(torch.float64) * (2.0 ** -32)    # below 2^63: non-negative as int64
        return out


def keep_count_of(keep_fraction, n):
    """ceil(keep_fraction * n), for a fraction in [0, 1]; a product within 1e-9 above an integer (0.1 * 30 in binary) counts as it."""
    f = float(keep_fraction)
    if not (0.0 <= f <= 1.0):
        raise ValueError(f"keep_fraction must be in [0, 1], got {keep_fraction!r}")
    return min(int(n), int(math.ceil(f * int(n) - 1e-9)))


def keep_mask(result, score="weight_sum", keep_fraction=None, keep_count=None, min_pixels=0):
    """The rows to keep, as a bool array like result[score] (a torch tensor on its device, or numpy).  Rows with pixels <
    min_pixels are dropped first; of the others the keep_count best by `score` stay (all of them if they are fewer), where
    keep_count = ceil(keep_fraction * N) over ALL N rows; equal scores are ordered by row index, the lower row first.  Exactly one
    of keep_fraction and keep_count may be given; neither: drop by min_pixels only.  Deterministic: a pure function of the result."""
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    if keep_fraction is not None and keep_count is not None:
        raise ValueError("keep_mask: give keep_fraction or keep_count, not both")
    values = result[score]
    as_torch = isinstance(values, torch.Tensor)
    v = values.detach().cpu().numpy() if as_torch else np.asarray(values)
    px = result["pixels"]
    px = px.detach().cpu().numpy() if isinstance(px, torch.Tensor) else np.asarray(px)
    n = int(v.shape[0])
    if px.shape != (n,) or v.shape != (n,):
        raise ValueError("keep_mask: the result's score and pixels must be [N]")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or int(min_pixels) < 0:
        raise ValueError(f"min_pixels must be an integer >= 0, got {min_pixels!r}")
    mask = px >= int(min_pixels)
    if keep_fraction is not None:
        keep_count = keep_count_of(keep_fraction, n)
    if keep_count is not None:
        if isinstance(keep_count, bool) or int(keep_count) != keep_count or not (0 <= int(keep_count) <= n):
            raise ValueError(f"keep_count must be an integer in [0, {n}], got {keep_count!r}")
        eligible = np.nonzero(mask)[0]
        if eligible.size > int(keep_count):
            order = np.argsort(-v[eligible].astype(np.float64), kind="stable")   # best first; ties: the lower row index first
            mask = np.zeros(n, bool)
            mask[eligible[order[:int(keep_count)]]] = True
    return torch.as_tensor(mask, device=values.device) if as_torch else mask


def compact(stepper, mask, strategy=None):
    """Keeps the rows of stepper.model where `mask` [N] is set: parameters, both Adam moments (brought up to date first: the lazily
    decayed moments belong to waves the rows leave), the lazy-moment wave steps and the stored permutation, through
    strategy._StateOps.keep as the strategies' own pruning; rows keep their order, so a spatial order survives.  strategy: a
    GSStrategy whose densification buffers follow the rows.  Returns the number of rows removed."""
    from .strategy import _StateOps
    raw = stepper.model.raw
    mask = torch.as_tensor(mask, dtype=torch.bool, device=raw.device)
    if tuple(mask.shape) != (raw.shape[0],):
        raise ValueError(f"compact: mask must be [{raw.shape[0]}], got {tuple(mask.shape)}")
    sync = getattr(stepper, "sync_moments", None)
    if sync is not None:
        sync()
    with torch.no_grad():
        _StateOps(stepper).keep(mask)
        accum = getattr(strategy, "grad_norm_accum", None)
        if accum is not None and accum.shape[0] == mask.shape[0]:
            m = mask.to(accum.device)
            strategy.grad_norm_accum, strategy.grad_norm_denom = accum[m], strategy.grad_norm_denom[m]
    return int(mask.numel() - int(mask.sum()))


# the trainer's `compaction` block
DEFAULTS = {"enabled": False, "keep_fraction": 0.5, "score": "weight_sum", "min_pixels": 1, "finetune_iterations": 0}
RULES = {"enabled": boolean(), "keep_fraction": number("in (0, 1]", gt=0, le=1), "score": one_of(SCORES), "min_pixels": integer(ge=0),
         "finetune_iterations": integer(ge=0)}


def check_config(block):
    """The resolved `compaction` block: enabled true or false, keep_fraction in (0, 1], score one of SCORES, min_pixels and
    finetune_iterations integers >= 0."""
    return check_block("compaction", block, DEFAULTS, RULES)
