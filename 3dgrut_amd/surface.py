"""The surface of a view: a distance and a Gaussian per pixel, and the scene as points.

Every other product of the walk says how much a Gaussian draws; this says where the surface is.  The forward's distance plane is
the un-normalised mean sum w * hitT and lies between surfaces wherever a ray crosses two of them.  SplatRaster.trace_surface
(gut_trace_surface) chooses ONE of the Gaussians the forward composited in a pixel and returns its hit distance, its index and its
blending weight:

    mode "level"        the first, in list order, behind which the transmittance is below `level`; 0.5 is the MEDIAN distance
    mode "max_weight"   the one with the largest blending weight w = T * alpha

`SurfaceRenderer` holds the model's rows activated and packed once (contribution.FrozenModel, as AttributeRenderer does) and renders
per view with one forward and the walk, nothing read back.  `backproject` turns a distance plane into world points, `fuse_points`
the median points of many views into one coloured cloud.  Render-only: nothing here has a gradient.  One GPU, the unsorted variant
at kernel degree 2.
"""
import math

import torch

from .confblock import boolean, check_block, integer, number
from .contribution import FrozenModel

# the trainer's `points` block: the median points (level 0.5) of every stride-th pixel of the training views, one per voxel of
# edge `voxel` (0: all of them).  stride and voxel are UNTUNED on real captures.
DEFAULTS = {"enabled": False, "level": 0.5, "stride": 1, "voxel": 0.0}
RULES = {"enabled": boolean(), "level": number("inside (0, 1)", gt=0, lt=1), "stride": integer(ge=1),
         "voxel": number("a finite edge length >= 0", ge=0)}


def check_config(block):
    """The resolved `points` block: enabled true or false, level inside (0, 1), stride an integer >= 1, voxel a finite edge >= 0."""
    return check_block("points", block, DEFAULTS, RULES)


class SurfaceRenderer(FrozenModel):
    """Renders the surface of `model` into the views handed to render(); the model must not change meanwhile."""

    def render(self, batch, mode="level", level=0.5):
        """dict(distance float32 [H,W] (0: none), id int64 [H,W] (-1: none), weight float32 [H,W], rgba [1,H,W,4] of the forward) of
        the batch's view: one forward plus one walk, nothing read back."""
        outs, rays_o, rays_d, cam = self.forward(batch)
        dist, ids, wgt = self.raster.trace_surface(0, self.n_active_features, self.act, rays_o, rays_d, *cam, mode=mode, level=level,
                                                   with_id=True, with_weight=True)
        return dict(distance=dist, id=ids, weight=wgt, rgba=outs[0])


def backproject(batch, distance):
    """[H,W,3] float32 world points of a distance plane [H,W]: T_to_world applied to rays_ori + distance * rays_dir (the hit
    distance is a length along the unit ray of the sensor frame).  A distance of 0 (no surface) gives NaN."""
    ro, rd = batch.rays_ori, batch.rays_dir
    H, W = int(ro.shape[1]), int(ro.shape[2])
    d = torch.as_tensor(distance, device=ro.device).to(torch.float32).reshape(H, W)
    d = torch.where(d > 0, d, torch.full_like(d, float("nan")))
    local = ro.reshape(H, W, 3).to(torch.float32) + d[..., None] * rd.reshape(H, W, 3).to(torch.float32)
    c2w = torch.as_tensor(batch.T_to_world, device=ro.device).to(torch.float32)
    c2w = c2w.reshape(-1, c2w.shape[-2], 4)[0]      # [1,4,4] or [1,3,4]
    return local @ c2w[:3, :3].T + c2w[:3, 3]


def fuse_points(renderer, batches, level=0.5, stride=1, voxel=0.0):
    """(xyz float32 [P,3], rgb float32 [P,3], id int64 [P]): the level-mode points of every stride-th pixel (rows and columns
    0, stride, 2 stride, ...) of every view that has a surface there, in view order and pixel order inside a view; rgb is the
    forward's colour at the pixel clamped to [0, 1], id the Gaussian.  voxel > 0: one point per occupied cell of that edge length
    (cell = floor(xyz / voxel)), the one that comes first in that order.  Deterministic; everything stays on the device."""
    stride, voxel = int(stride), float(voxel)
    if stride < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    if not (math.isfinite(voxel) and voxel >= 0.0):
        raise ValueError(f"voxel must be a finite edge length >= 0, got {voxel}")
    dev = renderer.act.device
    xyz, rgb, ids = [], [], []
    for batch in batches:
        r = renderer.render(batch, mode="level", level=level)
        H, W = r["distance"].shape
        keep = (r["id"][::stride, ::stride] >= 0).reshape(-1)
        xyz.append(backproject(batch, r["distance"])[::stride, ::stride].reshape(-1, 3)[keep])
        rgb.append(r["rgba"].reshape(H, W, 4)[::stride, ::stride, :3].reshape(-1, 3).clamp(0.0, 1.0)[keep])
        ids.append(r["id"][::stride, ::stride].reshape(-1)[keep])
    if not xyz:
        return (torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev), torch.zeros((0,), dtype=torch.int64, device=dev))
    xyz, rgb, ids = torch.cat(xyz), torch.cat(rgb), torch.cat(ids)
    if voxel > 0.0 and xyz.shape[0]:
        first = first_per_voxel(xyz, voxel)
        xyz, rgb, ids = xyz[first], rgb[first], ids[first]
    return xyz, rgb, ids


def first_per_voxel(xyz, voxel):
    """The indices, ascending, of the first point of every occupied cell floor(xyz / voxel)."""
    cells = torch.floor(xyz.to(torch.float64) / float(voxel)).to(torch.int64)
    occupied, inverse = torch.unique(cells, dim=0, return_inverse=True)
    order = torch.arange(xyz.shape[0], device=xyz.device)
    first = torch.full((occupied.shape[0],), xyz.shape[0], dtype=torch.int64, device=xyz.device)
    first.scatter_reduce_(0, inverse, order, reduce="amin")
    return torch.sort(first).values
