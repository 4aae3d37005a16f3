"""The scene as a triangle mesh: TSDF fusion of median-distance planes, surface nets on the fused volume.

surface.py gives a view a distance per pixel; this fuses the distance planes of many views into ONE signed distance field on a dense
axis-aligned grid and extracts its zero level.  Per view and voxel (gut_tsdf_integrate, one thread per voxel, up to
_capi.TSDF_MAX_VIEWS views a launch): the voxel centre is projected into the view by the projection kernel's arithmetic; with D the
pixel's distance and r the centre's distance from the pixel's ray origin, s = D - r is how far the centre lies in front of the
surface along the ray; centres more than `truncation` behind it are hidden and skipped, the others add min(1, s / truncation) in
units of 2^-16 to an int32 and 1 to a count.  Integer sums: the volume does not depend on the order of the views or on how they
are split into launches, and identical inputs give identical bytes.  `extract` runs surface nets on the integer state (one vertex per
cell with a sign change, one quad per lattice edge with a sign change, a defined order of both) with the per-cell and per-edge work
in HIP and the two scans in torch.  Render-only; one GPU, the unsorted variant at kernel degree 2 (the surface walk's scope).

`resolution`, `truncation_voxels` and the 1 % .. 99 % quantile box of volume_for are UNTUNED on real captures.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from .confblock import boolean, check_block, integer, is_number, nullable, number

# the trainer's `mesh` block.  voxel None: the longest edge of the box / resolution; bounds None: the quantile box of volume_for.
# resolution, truncation_voxels and the quantile box are UNTUNED on real captures.
DEFAULTS = {"enabled": False, "level": 0.5, "resolution": 256, "voxel": None, "truncation_voxels": 4, "min_count": 1, "bounds": None}

MAX_VOXELS = 1 << 30       # gut_hip.h: X Y Z <= 2^30
MAX_VIEWS = 32767          # acc is an int32 of quanta of 2^-16, at most 65536 a view
QUANTILES = (0.01, 0.99)


def check_bounds(bounds):
    """((x0, y0, z0), (x1, y1, z1)) as two float triples, lower corner strictly below the upper one."""
    try:
        lo, hi = bounds
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)), got {bounds!r}") from None
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi) or not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"bounds must be two finite corners, the first strictly below the second, got {bounds!r}")
    return lo, hi


_RESOLUTION = "an integer >= 2 truncation_voxels + 2"
RULES = {"enabled": boolean(), "level": number("inside (0, 1)", gt=0, lt=1), "truncation_voxels": number("finite and > 0", gt=0),
         "resolution": integer(words=_RESOLUTION), "voxel": nullable(number("a finite edge length > 0", gt=0)), "min_count": integer(ge=1)}


def check_config(block):
    """The resolved `mesh` block: enabled true or false, level inside (0, 1), resolution an integer >= 2 truncation_voxels + 2, voxel null
    or a finite edge > 0, truncation_voxels finite and > 0, min_count an integer >= 1, bounds null or two corners."""
    check_block("mesh", block, DEFAULTS, RULES)
    if int(block["resolution"]) < 2.0 * float(block["truncation_voxels"]) + 2.0:
        raise ValueError(f"mesh.resolution must be {_RESOLUTION}, got {block['resolution']!r}")
    if block["bounds"] is not None:
        check_bounds(block["bounds"])
    return block


def _plane(t, shape, what, dev):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.numel() == int(np.prod(shape))):
        raise ValueError(f"TSDFVolume.integrate: {what} must be a contiguous float32 tensor of {list(shape)} elements on {dev}")
    return t


class TSDFVolume:
    """A dense TSDF volume on `device`: voxel (i, j, k) of `dims` = (X, Y, Z) has its centre at origin + voxel * (i + 1/2, j + 1/2,
    k + 1/2); the state tensors are [Z,Y,X] (x fastest): acc int32, cnt int32 (the kernel's uint32 words), and with colours
    rgb_sum int32 [Z,Y,X,3], rgb_cnt int32 [Z,Y,X].  All zero = empty."""

    def __init__(self, origin, voxel, dims, truncation, colours=True, device="cuda:0"):
        origin = [float(v) for v in origin]
        dims = [int(v) for v in dims]
        voxel, truncation = float(voxel), float(truncation)
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
            raise ValueError(f"TSDFVolume: origin must be three finite numbers, got {origin!r}")
        if not (math.isfinite(voxel) and voxel > 0.0) or not (math.isfinite(truncation) and truncation > 0.0):
            raise ValueError(f"TSDFVolume: voxel and truncation must be finite and > 0, got {voxel!r} and {truncation!r}")
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise ValueError(f"TSDFVolume: dims must be three integers >= 1 with X Y Z <= 2^30, got {dims!r}")
        self.origin, self.voxel, self.dims, self.truncation = tuple(origin), voxel, tuple(dims), truncation
        self.device = torch.device(device)
        X, Y, Z = dims
        self.acc = torch.zeros((Z, Y, X), dtype=torch.int32, device=self.device)
        self.cnt = torch.zeros((Z, Y, X), dtype=torch.int32, device=self.device)
        self.rgb_sum = torch.zeros((Z, Y, X, 3), dtype=torch.int32, device=self.device) if colours else None
        self.rgb_cnt = torch.zeros((Z, Y, X), dtype=torch.int32, device=self.device) if colours else None
        self.n_views = 0

    # ---- the C records ----
    def _grid(self):
        g = _capi.GutTsdfGrid()
        g.origin[:] = self.origin
        g.voxel = self.voxel
        g.dims[:] = self.dims
        g.truncation = self.truncation
        g.d_acc, g.d_cnt = self.acc.data_ptr(), self.cnt.data_ptr()
        g.d_rgb_sum = None if self.rgb_sum is None else self.rgb_sum.data_ptr()
        g.d_rgb_cnt = None if self.rgb_cnt is None else self.rgb_cnt.data_ptr()
        return g

    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume: integration and extraction run on a GPU; there is no CPU path")
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def integrate(self, views):
        """Adds `views`, any number of them, _capi.TSDF_MAX_VIEWS a launch.  A view is a dict: camera (a _capi.GutCamera with
        pose_start == pose_end), distance (float32 [H,W] on the device, 0: no surface), optionally rgba (the forward's [..,H,W,4])
        and ray_origin ([..,H,W,3] in the sensor frame; None: the rays start at the sensor position).  Returns self."""
        views = list(views)
        if self.n_views + len(views) > MAX_VIEWS:
            raise ValueError(f"TSDFVolume.integrate: {self.n_views} + {len(views)} views pass {MAX_VIEWS}, the most an int32 of "
                             "2^-16 quanta holds")
        lib, grid = _capi.load(), self._grid()
        for at in range(0, len(views), _capi.TSDF_MAX_VIEWS):
            batch = views[at:at + _capi.TSDF_MAX_VIEWS]
            records = (_capi.GutTsdfView * len(batch))()
            keep = []
            for rec, v in zip(records, batch):
                dist = v["distance"]
                if not (isinstance(dist, torch.Tensor) and dist.dim() == 2):
                    raise ValueError("TSDFVolume.integrate: distance must be a [H,W] tensor")
                H, W = int(dist.shape[0]), int(dist.shape[1])
                cam = v["camera"]
                if not isinstance(cam, _capi.GutCamera):
                    raise ValueError("TSDFVolume.integrate: camera must be a _capi.GutCamera (view_of builds one from a batch)")
                rec.camera = C.pointer(cam)
                rec.width, rec.height = W, H
                rec.d_distance = _plane(dist, (H, W), "distance", self.device).data_ptr()
                rgba, origin = v.get("rgba"), v.get("ray_origin")
                rec.d_rgba = None if rgba is None else _plane(rgba, (H, W, 4), "rgba", self.device).data_ptr()
                rec.d_ray_origin = None if origin is None else _plane(origin, (H, W, 3), "ray_origin", self.device).data_ptr()
                keep.append((cam, dist, rgba, origin))
            with torch.cuda.device(self.device):
                rc = lib.gut_tsdf_integrate(self._stream(), C.byref(grid), len(batch), records)
            _capi.check(rc, "tsdf_integrate")
            self.n_views += len(batch)
        return self

    def tsdf(self):
        """float32 [Z,Y,X]: acc / (cnt * 65536), the mean truncated signed distance in units of the truncation; NaN where no view
        updated the voxel."""
        cnt = self.cnt.to(torch.float32)
        return torch.where(self.cnt != 0, self.acc.to(torch.float32) / (cnt * 65536.0), torch.full_like(cnt, float("nan")))

    def extract(self, min_count=1):
        """(vertices float32 [V,3] in the world, colours float32 [V,3], faces int32 [F,3]) of the zero level by surface nets, on the
        device.  A lattice point counts as observed with cnt >= min_count.  Vertices are ordered by cell, quads by lattice point and
        axis, each quad as two triangles whose normal points from inside (acc < 0) to outside.  One host read (the two counts)."""
        if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
            raise ValueError(f"min_count must be an integer >= 1, got {min_count!r}")
        lib, grid, stream = _capi.load(), self._grid(), self._stream()
        n = self.acc.numel()
        cell = torch.empty((n,), dtype=torch.uint8, device=self.device)
        quads = torch.empty((n,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(lib.gut_surface_nets_count(stream, C.byref(grid), int(min_count), cell.data_ptr(), quads.data_ptr()), "surface_nets_count")
            active = (cell >> 1).to(torch.int32)
            vertex_offset = torch.cumsum(active, 0, dtype=torch.int32)
            quad_offset = torch.cumsum(quads, 0, dtype=torch.int32)
            n_vertices, n_quads = (int(v) for v in torch.stack([vertex_offset[-1], quad_offset[-1]]).cpu())
            vertex_offset -= active                     # exclusive
            quad_offset -= quads.to(torch.int32)
            vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=self.device)
            colours = torch.empty((n_vertices, 3), dtype=torch.float32, device=self.device)
            faces = torch.empty((2 * n_quads, 3), dtype=torch.int32, device=self.device)
            if n_vertices:
                # (an empty tensor's data_ptr is 0: with no quad the faces are written nowhere, but the entry point wants a pointer)
                spare = torch.empty((4,), dtype=torch.int32, device=self.device)
                _capi.check(lib.gut_surface_nets_emit(stream, C.byref(grid), int(min_count), cell.data_ptr(), quads.data_ptr(),
                                                      vertex_offset.data_ptr(), quad_offset.data_ptr(), vertices.data_ptr(), colours.data_ptr(),
                                                      faces.data_ptr() if n_quads else spare.data_ptr()), "surface_nets_emit")
        return vertices, colours, faces


def _quantile_box(positions):
    """(lo, hi) float lists: per axis the values at the 1 % and 99 % ranks of the sorted coordinates (floor and ceil of q (n - 1))."""
    pos = torch.as_tensor(positions).detach().to(torch.float32).reshape(-1, 3)
    n = int(pos.shape[0])
    if n < 1:
        raise ValueError("volume_for: the model has no rows")
    ordered = torch.sort(pos, dim=0).values
    lo = ordered[int(math.floor(QUANTILES[0] * (n - 1) + 1e-9))]      # (0.99 * 20000 is not 19800 in binary)
    hi = ordered[int(math.ceil(QUANTILES[1] * (n - 1) - 1e-9))]
    return [float(v) for v in lo.cpu()], [float(v) for v in hi.cpu()]


def volume_for(model, resolution=256, voxel=None, bounds=None, truncation_voxels=4, colours=True, device=None):
    """A TSDFVolume for `model`.  bounds None: the box of model.positions between the 1 % and 99 % quantile per axis, grown by the
    truncation on every side; else ((x0, y0, z0), (x1, y1, z1)) as it is.  voxel None: the longest edge of that box / resolution
    (for the grown box: voxel = longest quantile edge / (resolution - 2 truncation_voxels), so that the grown edge is resolution
    voxels).  truncation = truncation_voxels * voxel; dims = ceil(edge / voxel) per axis, at least 2."""
    resolution, tv = int(resolution), float(truncation_voxels)
    if not (math.isfinite(tv) and tv > 0.0):
        raise ValueError(f"volume_for: truncation_voxels must be finite and > 0, got {truncation_voxels!r}")
    if voxel is not None and not (is_number(voxel) and float(voxel) > 0.0):
        raise ValueError(f"volume_for: voxel must be a finite edge length > 0, got {voxel!r}")
    if bounds is not None:
        lo, hi = check_bounds(bounds)
        if voxel is None:
            if resolution < 2:
                raise ValueError(f"volume_for: resolution must be >= 2, got {resolution}")
            voxel = max(b - a for a, b in zip(lo, hi)) / resolution
    else:
        lo, hi = _quantile_box(model.positions)
        longest = max(b - a for a, b in zip(lo, hi))
        if voxel is None:
            if resolution < 2.0 * tv + 2.0:
                raise ValueError(f"volume_for: resolution must be >= 2 truncation_voxels + 2, got {resolution}")
            if not longest > 0.0:
                raise ValueError("volume_for: the model's quantile box is empty; give bounds or voxel")
            voxel = longest / (resolution - 2.0 * tv)
        grow = tv * float(voxel)
        lo, hi = [a - grow for a in lo], [b + grow for b in hi]
    voxel = float(voxel)
    dims = [max(2, int(math.ceil((b - a) / voxel - 1e-6))) for a, b in zip(lo, hi)]
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"volume_for: {dims} voxels pass 2^30; choose a larger voxel or a smaller box")
    if device is None:
        device = torch.as_tensor(model.positions).device
    return TSDFVolume(lo, voxel, dims, tv * voxel, colours=colours, device=device)


def view_of(batch, render):
    """The integrate() view of a batch and SurfaceRenderer.render's dict for it: the camera at the batch's pose, the distance plane,
    the forward's colours, and the ray-origin plane if some ray of the batch does not start at the sensor position."""
    from .tracer import SplatRaster, Tracer, _pose_args
    sensor, poses = Tracer.create_camera_parameters(batch)
    cam = SplatRaster._camera(sensor, *_pose_args(poses))
    dist = render["distance"].contiguous()
    H, W = int(dist.shape[0]), int(dist.shape[1])
    origin = batch.rays_ori.to(torch.float32).reshape(H, W, 3).contiguous()
    return dict(camera=cam, distance=dist, rgba=render["rgba"].reshape(H, W, 4).contiguous(),
                ray_origin=origin if bool((origin != 0).any()) else None)


def fuse_mesh(renderer, batches, volume, level=0.5):
    """Integrates the level-mode surface (level 0.5: the median distance) of every batch into `volume`: per view one
    SurfaceRenderer.render, the views of a launch integrated together.  Returns the volume."""
    pending = []
    for batch in batches:
        pending.append(view_of(batch, renderer.render(batch, mode="level", level=level)))
        if len(pending) == _capi.TSDF_MAX_VIEWS:
            volume.integrate(pending)
            pending = []
    if pending:
        volume.integrate(pending)
    return volume
