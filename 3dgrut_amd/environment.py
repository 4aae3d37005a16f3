"""A learnt radiance at infinity: a cube-map background behind the Gaussians.

The Gaussians carry everything the model knows about a scene; what lies behind them was one colour.  `EnvironmentMap` holds a
direction-indexed map, texels [6,R,R,3] float32 (plain RGB, unconstrained, like the SH colours), its Adam state, and the buffers
of its two kernels:

    plane = env.plane(batch)                          # [H,W,3]: gut_environment_sample, no graph; the fused loss's background
    env.backward_from_loss(batch, rgba, rgba_grad)    # texels.grad from the fused loss's own output: c = (1 - alpha) g_rgb
    env.step()                                        # torch.optim.Adam on the texels, same stream

    env.sample(rays_dir, T_to_world)                  # the same plane under autograd (the torch loss branch, evaluation)

The plane of a pixel depends on the camera-space ray and on the camera-to-world ROTATION alone: the nine floats the compositors
apply to a ray (gut_environment_rotation builds them from the view's pose exactly as the trace calls do), so a refined pose is
covered when the posed batch is passed.  The pose gets no gradient from the map.  The adjoint sums integers (§13, §14, §17):
identical inputs give identical bits.  Nothing is copied to the host and nothing waits.
"""
import ctypes as C
import math

import numpy as np
import torch

from .confblock import boolean, check_block, integer, nullable, number

DEFAULTS = {"enabled": False, "resolution": 256, "lr": 0.01, "init": 0.5, "start_iteration": 0, "end_iteration": None}
MAX_RESOLUTION = 8192   # _capi.ENVIRONMENT_MAX_RESOLUTION: 18 R^2 stays below 2^31
RULES = {"enabled": boolean(), "resolution": (lambda v: integer(ge=1)[0](v) and int(v) <= MAX_RESOLUTION, f"an integer in 1 .. {MAX_RESOLUTION}"),
         "lr": number("finite and >= 0", ge=0), "init": number("finite"), "start_iteration": integer(ge=0),
         "end_iteration": nullable(integer(ge=0))}


def check_config(block):
    """The resolved `environment` block: resolution 1 .. 8192, rate finite and >= 0, init finite, start_iteration >= 0,
    end_iteration null (to the end of the run) or >= 0."""
    return check_block("environment", block, DEFAULTS, RULES)


def rotation_from_pose(T_to_world, poses=None):
    """The nine floats M (numpy float32 [9], row-major camera-to-world rotation) the compositors apply to the rays of the view with
    the camera-to-world matrix T_to_world: through the same pose conversion as Tracer.create_camera_parameters and the library's
    own construction of the view.  poses: that conversion's SensorPose3D, where the caller has it already."""
    from . import _capi
    if poses is None:
        from .pose import sensor_pose_from_c2w
        T = T_to_world.detach().cpu().numpy() if isinstance(T_to_world, torch.Tensor) else np.asarray(T_to_world)
        poses = sensor_pose_from_c2w(T.reshape(4, 4))
    cam = _capi.GutCamera()
    cam.pose_start[:] = np.asarray(poses.T_world_sensors[0], np.float32).reshape(7).tolist()
    cam.pose_end[:] = np.asarray(poses.T_world_sensors[1], np.float32).reshape(7).tolist()
    out = (C.c_float * 9)()
    _capi.check(_capi.load().gut_environment_rotation(C.byref(cam), out), "environment_rotation")
    return np.array(out[:], dtype=np.float32)


class _Sample(torch.autograd.Function):
    """plane = sample(texels): the graph reaches the texels only; the backward is the plane-cotangent form of the adjoint."""

    @staticmethod
    def forward(ctx, texels, env, rays_dir, M):
        ctx.env, ctx.rays_dir, ctx.M = env, rays_dir, M
        return env._sample(rays_dir, M, torch.empty(rays_dir.shape[-3:-1] + (3,), dtype=torch.float32, device=rays_dir.device))

    @staticmethod
    def backward(ctx, plane_grad):
        grad = torch.empty_like(ctx.env.texels)
        ctx.env._backward(ctx.rays_dir, ctx.M, grad, plane_grad=plane_grad.contiguous())
        return grad, None, None, None


class EnvironmentMap:
    def __init__(self, resolution=DEFAULTS["resolution"], init=DEFAULTS["init"], device="cuda", lr=DEFAULTS["lr"], start_iteration=0,
                 end_iteration=None):
        R = int(resolution)
        if not 1 <= R <= MAX_RESOLUTION:
            raise ValueError(f"EnvironmentMap: resolution must be 1 .. {MAX_RESOLUTION}, got {resolution!r}")
        self.device = torch.device(device)
        self.resolution = R
        self.texels = torch.full((6, R, R, 3), float(init), dtype=torch.float32, device=self.device)
        self.optimizer = torch.optim.Adam([self.texels], lr=float(lr))
        self.start_iteration, self.end_iteration = int(start_iteration), (None if end_iteration is None else int(end_iteration))
        self._lib, self._workspace, self._plane, self._grad = None, None, None, None
        if self.device.type == "cuda":
            from . import _capi
            self._lib = _capi.load()
            self._workspace = torch.empty(((self._lib.gut_environment_workspace_bytes(R) + 7) // 8,), dtype=torch.int64, device=self.device)
            self._grad = torch.empty_like(self.texels)

    def active(self, step):
        """Whether iteration `step` updates the map (start_iteration <= step < end_iteration; null: no end).  Outside, the map is
        still composited and nothing is scattered or stepped."""
        return step >= self.start_iteration and (self.end_iteration is None or step < self.end_iteration)

    # ---- the two kernels ----
    def _view(self, rays_dir, M):
        from . import _capi
        if rays_dir.dtype != torch.float32 or rays_dir.device != self.texels.device or not rays_dir.is_contiguous() or rays_dir.shape[-1] != 3 \
                or rays_dir.dim() not in (3, 4) or (rays_dir.dim() == 4 and rays_dir.shape[0] != 1):
            raise ValueError(f"EnvironmentMap: rays_dir must be a contiguous float32 [H,W,3] or [1,H,W,3] tensor on {self.texels.device}, "
                             f"got {tuple(rays_dir.shape)} {rays_dir.dtype} on {rays_dir.device}")
        if self._lib is None:
            raise RuntimeError("EnvironmentMap: the map is sampled by the HIP library; this one lives on the host")
        H, W = int(rays_dir.shape[-3]), int(rays_dir.shape[-2])
        view = _capi.GutEnvironmentView(rays_dir.data_ptr(), (C.c_float * 9)(*[float(x) for x in np.asarray(M, np.float32).reshape(9)]), H, W)
        return view, H, W

    def _sample(self, rays_dir, M, out):
        from . import _capi
        view, _, _ = self._view(rays_dir, M)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            rc = self._lib.gut_environment_sample(C.c_void_p(stream), C.byref(view), self.texels.data_ptr(), self.resolution, out.data_ptr())
        _capi.check(rc, "environment_sample")
        return out

    def _backward(self, rays_dir, M, grad, plane_grad=None, rgba=None, rgba_grad=None):
        from . import _capi
        view, H, W = self._view(rays_dir, M)
        for name, t, c in (("plane_grad", plane_grad, 3), ("rgba", rgba, 4), ("rgba_grad", rgba_grad, 4)):
            if t is not None and (t.dtype != torch.float32 or t.device != self.texels.device or not t.is_contiguous() or t.numel() != H * W * c):
                raise ValueError(f"EnvironmentMap: {name} must be a contiguous float32 [{H},{W},{c}] tensor on {self.texels.device}")
        ptr = lambda t: None if t is None else t.data_ptr()
        cot = _capi.GutEnvironmentCotangent(ptr(plane_grad), ptr(rgba), ptr(rgba_grad))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            rc = self._lib.gut_environment_backward(C.c_void_p(stream), C.byref(view), C.byref(cot), self.resolution,
                                                    self._workspace.data_ptr(), grad.data_ptr())
        _capi.check(rc, "environment_backward")
        return grad

    # ---- the public surface ----
    def plane(self, batch, poses=None):
        """The [H,W,3] background plane of the batch's view, no graph: a buffer of this object, rewritten by the next call."""
        rays = batch.rays_dir.contiguous()
        H, W = int(rays.shape[-3]), int(rays.shape[-2])
        if self._plane is None or tuple(self._plane.shape) != (H, W, 3):
            self._plane = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        return self._sample(rays, rotation_from_pose(batch.T_to_world, poses), self._plane)

    def sample(self, rays_dir, T_to_world, poses=None):
        """The plane of rays_dir [H,W,3] / [1,H,W,3] under the camera-to-world matrix T_to_world, a fresh [H,W,3] tensor.  With
        texels.requires_grad the graph reaches the texels (and only them); without, no graph and the same bits."""
        rays = rays_dir.detach().contiguous()
        M = rotation_from_pose(T_to_world, poses)
        if self.texels.requires_grad and torch.is_grad_enabled():
            return _Sample.apply(self.texels, self, rays, M)
        return self._sample(rays, M, torch.empty(rays.shape[-3:-1] + (3,), dtype=torch.float32, device=self.device))

    def backward_from_loss(self, batch, rgba, rgba_grad, poses=None):
        """texels.grad from the fused loss's output of the batch's view: the loss composited rgb + B (1 - alpha) and left
        d loss / d comp in the rgb channels of rgba_grad (mask and exposure folded in), so d loss / d B = (1 - alpha) rgba_grad.rgb,
        formed inside the scatter.  Every element of texels.grad is written."""
        self._backward(batch.rays_dir.contiguous(), rotation_from_pose(batch.T_to_world, poses), self._grad, rgba=rgba, rgba_grad=rgba_grad)
        self.texels.grad = self._grad
        return self._grad

    def step(self):
        """One Adam step on the texels from texels.grad, on the current stream."""
        self.optimizer.step()

    def state_dict(self):
        """Tensors only (a checkpoint's `native` block must load with weights_only=True): texels, Adam's moments and step count."""
        st = self.optimizer.state.get(self.texels, {})
        zeros = lambda: torch.zeros_like(self.texels, device="cpu")
        return dict(texels=self.texels.detach().cpu().clone(),
                    exp_avg=st["exp_avg"].detach().cpu().clone() if "exp_avg" in st else zeros(),
                    exp_avg_sq=st["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in st else zeros(),
                    step=torch.as_tensor(st["step"]).detach().cpu().to(torch.float32).reshape(()).clone() if "step" in st else torch.zeros(()))

    def load_state_dict(self, state):
        texels = state["texels"]
        if tuple(texels.shape) != tuple(self.texels.shape):
            raise ValueError(f"EnvironmentMap.load_state_dict: the checkpoint holds a map of resolution {tuple(texels.shape)[1]}, this run "
                             f"has {self.resolution}")
        self.texels.copy_(texels)
        self.optimizer.state.pop(self.texels, None)
        if float(state["step"]) > 0:   # (a map that never stepped has no Adam state: the first step creates it)
            self.optimizer.state[self.texels] = dict(step=state["step"].detach().to(torch.float32).reshape(()).clone(),
                                                     exp_avg=state["exp_avg"].to(self.device).clone(),
                                                     exp_avg_sq=state["exp_avg_sq"].to(self.device).clone())

    def mean_colour(self):
        """[r, g, b]: the mean of the texels (reads the map back: end of run)."""
        return [float(x) for x in self.texels.detach().reshape(-1, 3).mean(0).cpu()]

    def to_equirect(self, height):
        """A lat-long float image [height, 2 height, 3] of the map, for looking at it: row 0 is +y, the columns run round y and the centre column looks along -z.
        Plain torch with §20's face and texel rules (nearest rounding differences aside); not a training path."""
        Hh, Ww, R = int(height), 2 * int(height), self.resolution
        lat = (0.5 - (torch.arange(Hh, dtype=torch.float32, device=self.device) + 0.5) / Hh) * math.pi
        lon = ((torch.arange(Ww, dtype=torch.float32, device=self.device) + 0.5) / Ww * 2.0 - 1.0) * math.pi
        e = torch.stack([torch.cos(lat)[:, None] * torch.sin(lon)[None, :], torch.sin(lat)[:, None].expand(Hh, Ww),
                         -torch.cos(lat)[:, None] * torch.cos(lon)[None, :]], dim=-1).reshape(-1, 3)
        a = e.abs()
        axis = torch.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, torch.where(a[:, 1] >= a[:, 2], 1, 2))
        pick = lambda k: e.gather(1, ((axis + k) % 3)[:, None])[:, 0]
        m = pick(0).abs()
        face = 2 * axis + (pick(0) < 0).long()
        s, t = (pick(1) / m + 1.0) * (0.5 * R) - 0.5, (pick(2) / m + 1.0) * (0.5 * R) - 0.5
        i0, j0 = torch.floor(s), torch.floor(t)
        fx, fy = (s - i0)[:, None], (t - j0)[:, None]
        c0, c1 = i0.long().clamp(0, R - 1), (i0.long() + 1).clamp(0, R - 1)
        r0, r1 = j0.long().clamp(0, R - 1), (j0.long() + 1).clamp(0, R - 1)
        T = self.texels.detach()
        img = ((1 - fx) * (1 - fy) * T[face, r0, c0] + fx * (1 - fy) * T[face, r0, c1]) + (1 - fx) * fy * T[face, r1, c0] + fx * fy * T[face, r1, c1]
        return img.reshape(Hh, Ww, 3)
