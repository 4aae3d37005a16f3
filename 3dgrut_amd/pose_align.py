"""Pose alignment of held-out views before they are scored.

A run with `pose_refinement` on moves the training cameras and the Gaussians follow them; the held-out cameras stay where the SfM
solution put them, so their PSNR charges the model for a sub-pixel misregistration it was asked to remove.  As every pose-refining
method does before it scores a held-out view (BARF, CamP, Zip-NeRF), `PoseAligner` optimises that view's pose against its photo with
the model FROZEN and hands back the pose at which the photometric loss was smallest:

    T_0 = the given camera-to-world matrix (float64, host), Adam moments and visit count zero
    k = 0 .. K-1:  render at T_k;  l_k = L(T_k);  pose-only backward of dL/d rgba -> out8;  six-float Adam -> delta_k;
                   T_{k+1} = pose.apply_pose_increment(T_k, delta_k)
    one more render and loss: l_K
    the aligned pose is T_{k*}, k* the SMALLEST index of the smallest finite l_k (k* = 0 when l_0 is not finite)

so loss_aligned <= loss_given by construction, whatever the photo, and K = 0 returns the given matrix bit for bit.  L is the run's
fused photometric loss (lambda_l1 / lambda_ssim) over the model's evaluation background; a batch's mask enters L and never a score.

The step that turns a batch into (loss, out8) is a callable handed to the aligner.  `DeviceStep` is the product's: SplatRaster.trace
on rows activated and packed ONCE per pass, the fused loss, and SplatRaster.trace_bwd_pose (gut_trace_bwd_pose), the backward that
runs the compositor and a consuming form of the pose reduction and nothing else, so no [N,...] gradient tensor exists at any point.
With device tensors the Adam is gut_pose_adam_step and an iteration costs two small device-to-host copies (increment, loss) behind
one synchronisation: the next camera is built on the host.  With host tensors (tests) the same arithmetic runs in torch.

`lr_translation` is in world units here (the trainer multiplies its setting by the scene extent), `lr_rotation` in radians.  The
default rates and iteration count are those of the pose-refinement defaults and of the project's recovery test: UNTUNED on real
captures.  Only views with a single pose can be aligned; rolling-shutter views and data-parallel evaluation are out of scope.
"""
import copy
import ctypes as C

import numpy as np
import torch

from .confblock import boolean, check_block, integer, number
from .pose import apply_pose_increment, pose_difference

DEFAULTS = {"enabled": False, "validation": False, "iterations": 50, "lr_translation": 0.001, "lr_rotation": 0.0005,
            "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}
_RATE, _BETA = number("finite and >= 0", ge=0), number("in [0, 1)", ge=0, lt=1)
RULES = {"enabled": boolean(), "validation": boolean(), "iterations": integer(ge=0), "lr_translation": _RATE, "lr_rotation": _RATE,
         "eps": _RATE, "beta1": _BETA, "beta2": _BETA}


def check_config(block):
    """The resolved `pose_alignment` block: enabled / validation true or false, iterations an integer >= 0, rates and eps finite and
    >= 0, betas in [0, 1)."""
    return check_block("pose_alignment", block, DEFAULTS, RULES)


def _single_pose(batch):
    """The batch's one camera-to-world matrix as float64 [4,4]; ValueError for a view with two poses (T_to_world_end differing from
    T_to_world, or more than one matrix in T_to_world): the pose gradient is defined for pose_start == pose_end only."""
    T = np.asarray(torch.as_tensor(batch.T_to_world).detach().cpu().numpy(), np.float64)
    if T.size != 16:
        raise ValueError(f"PoseAligner: a view needs ONE camera-to-world matrix, T_to_world has shape {tuple(T.shape)}")
    T = T.reshape(4, 4)
    end = getattr(batch, "T_to_world_end", None)
    if end is not None:
        E = np.asarray(torch.as_tensor(end).detach().cpu().numpy(), np.float64)
        if E.size != 16 or not np.array_equal(E.reshape(4, 4), T):
            raise ValueError("PoseAligner: the view's start and end poses differ: only views with a single pose can be aligned")
    return T


class DeviceStep:
    """batch -> (loss [1], out8 [8]) on the GPU with the model frozen.  The [N,12] activated rows and the [N,48] features are
    prepared here, once; a pass over many views and iterations reuses them.  `out8` is this object's own buffer; while a call runs
    it is the handle's pose output, and `release()` puts back what the handle had before `acquire()`."""

    def __init__(self, model, tracer, lambda_l1=0.8, lambda_ssim=0.2):
        from . import _capi
        from .tracer import Tracer
        self._lib = _capi.load()
        self._create_camera = Tracer.create_camera_parameters
        self.raster = tracer.tracer_wrapper
        with torch.no_grad():
            z = torch.zeros_like(model.get_density())
            self.act = torch.cat([model.positions, model.get_density(), model.get_rotation(), model.get_scale(), z], dim=1).to(torch.float32).contiguous()
            self.features = model.get_features().detach().to(torch.float32).contiguous()
        self.n_active_features = int(model.n_active_features)
        # the evaluation background: black or white; `random` composites nothing at evaluation, i.e. black (evaluate.py)
        self.background = 1.0 if getattr(model, "background_color", "black") == "white" else 0.0
        self.lambda_l1, self.lambda_ssim = float(lambda_l1), float(lambda_ssim)
        self.out8 = torch.zeros(8, dtype=torch.float32, device=self.act.device)
        self._ws = None
        self._previous = None
        self._acquired = False

    def acquire(self):
        if not self._acquired:
            self._previous = getattr(self.raster, "_pose_out", None)
            self.raster.set_pose_gradient(self.out8)
            self._acquired = True

    def release(self):
        if self._acquired:
            self._acquired = False
            self.raster.set_pose_gradient(self._previous)
            self._previous = None
            self.raster.collect_times()   # the aligner's forwards and backwards leave no sample behind for the next scoring render

    def forward_loss(self, batch):
        """(loss3, rgba_grad, trace arguments, rgba, dist) of the render at the batch's pose."""
        from .losses import _photometric_loss_call, _plane_mask
        sensor, poses = self._create_camera(batch)
        rays_o, rays_d = batch.rays_ori.contiguous(), batch.rays_dir.contiguous()
        cam = (sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
        rgba, dist, _, _ = self.raster.trace(0, self.n_active_features, self.act, self.features, rays_o, rays_d, None, *cam)
        H, W = int(rgba.shape[0]), int(rgba.shape[1])
        gt = batch.rgb_gt
        if gt.dtype != torch.float32 or not gt.is_contiguous() or gt.device != rgba.device:
            gt = gt.to(device=rgba.device, dtype=torch.float32).contiguous()
        need = self._lib.gut_photometric_workspace_bytes(H, W)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=rgba.device)
        mask = getattr(batch, "mask", None)
        with torch.cuda.device(rgba.device):
            loss3, rgba_grad = _photometric_loss_call(self._lib, H, W, rgba, gt, self.background, self.lambda_l1, self.lambda_ssim,
                                                      None if mask is None else _plane_mask(mask, H, W, rgba.device), self._ws)
        return loss3, rgba_grad, (rays_o, rays_d, *cam), rgba, dist

    def loss(self, batch):
        return self.forward_loss(batch)[0][0:1]

    def __call__(self, batch):
        loss3, rgba_grad, args, rgba, dist = self.forward_loss(batch)
        self.raster.trace_bwd_pose(0, self.n_active_features, self.act, *args, rgba, rgba_grad, dist, None)
        return loss3[0:1], self.out8


class PoseAligner:
    def __init__(self, step, iterations=50, lr_translation=0.001, lr_rotation=0.0005, betas=(0.9, 0.999), eps=1e-15, loss_only=None):
        """step: callable(batch) -> (loss, out8): the photometric loss of the render at batch.T_to_world (a number or a tensor of one
        element) and the pose gradient {F[3], M[3], rows, 0} of that loss (dL/d rho = -F, dL/d phi = -M), both on one device.
        loss_only: callable(batch) -> loss for the last evaluation, which needs no gradient (default: step's loss).  A step with
        acquire() / release() (DeviceStep) is bracketed by them in every align()."""
        if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 0:
            raise ValueError(f"PoseAligner: iterations must be an integer >= 0, got {iterations!r}")
        self.step = step
        self.loss_only = loss_only if loss_only is not None else getattr(step, "loss", None)
        self.iterations = int(iterations)
        self.lr_translation, self.lr_rotation = float(lr_translation), float(lr_rotation)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self._dev = None   # device state (moments, count, increment) and its pinned host slot, built at the first device gradient

    def _device_state(self, device):
        if self._dev is None or self._dev["m"].device != device:
            from . import _capi
            z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=device)
            self._dev = dict(m=z(6), v=z(6), count=z(1, torch.int32), delta=z(6), slot=torch.zeros(7, dtype=torch.float32).pin_memory(),
                             lib=_capi.load(), check=_capi.check)
        return self._dev

    def _adam_device(self, grad8, loss):
        """gut_pose_adam_step, then the increment and the loss into the pinned slot: two copies, one synchronisation."""
        d = self._device_state(grad8.device)
        stream = torch.cuda.current_stream(grad8.device)
        with torch.cuda.device(grad8.device):
            d["check"](d["lib"].gut_pose_adam_step(C.c_void_p(stream.cuda_stream), grad8.data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                                                   d["count"].data_ptr(), self.lr_translation, self.lr_rotation, self.betas[0],
                                                   self.betas[1], self.eps, d["delta"].data_ptr()), "pose_adam_step")
            d["slot"][0:6].copy_(d["delta"], non_blocking=True)
            d["slot"][6:7].copy_(loss.detach().reshape(1).to(torch.float32), non_blocking=True)
            stream.synchronize()
        return d["slot"][0:6].numpy().astype(np.float64), float(d["slot"][6])

    def _adam_host(self, state, grad8):
        """PoseRefiner's host-tensor form: the kernel's arithmetic in float32, the betas and 1 - beta held in float32."""
        b1, b2 = float(np.float32(self.betas[0])), float(np.float32(self.betas[1]))
        c1, c2 = float(np.float32(1) - np.float32(self.betas[0])), float(np.float32(1) - np.float32(self.betas[1]))
        g = -torch.as_tensor(grad8)[:6].detach().to("cpu", torch.float32)
        state["count"] += 1
        t = float(state["count"])
        m, v = state["m"], state["v"]
        m.mul_(b1).add_(g, alpha=c1)
        v.mul_(b2).addcmul_(g, g, value=c2)
        lr = torch.tensor([self.lr_translation] * 3 + [self.lr_rotation] * 3, dtype=torch.float32)
        delta = -lr * (m / (1.0 - b1 ** t)) / ((v / (1.0 - b2 ** t)).sqrt() + self.eps)
        return delta.numpy().astype(np.float64)

    @staticmethod
    def _at(batch, T):
        out = copy.copy(batch)
        out.T_to_world = torch.as_tensor(T, dtype=torch.float32).reshape(1, 4, 4)   # a host tensor: the camera is built on the host
        return out

    def align(self, batch):
        """dict(pose [4,4] float64, losses [K+1], best_iteration, loss_given, loss_aligned, translation, rotation_deg (the aligned
        pose against the given one))."""
        T0 = _single_pose(batch)     # raises before any launch
        acquire, release = getattr(self.step, "acquire", None), getattr(self.step, "release", None)
        if acquire is not None:
            acquire()
        try:
            poses, losses = [T0], []
            host = dict(m=torch.zeros(6), v=torch.zeros(6), count=0)
            if self._dev is not None:
                for k in ("m", "v", "count"):
                    self._dev[k].zero_()
            T = T0
            for _ in range(self.iterations):
                loss, grad8 = self.step(self._at(batch, T))
                if isinstance(grad8, torch.Tensor) and grad8.is_cuda:
                    delta, value = self._adam_device(grad8, loss)
                else:
                    delta, value = self._adam_host(host, grad8), float(loss)
                losses.append(value)
                if not np.isfinite(delta).all():   # a non-finite gradient moves nothing (and poisons nothing that follows)
                    delta = np.zeros(6)
                T = apply_pose_increment(T, delta)
                poses.append(T)
            last = self.loss_only(self._at(batch, T)) if self.loss_only is not None else self.step(self._at(batch, T))[0]
            losses.append(float(last))   # (a device tensor: the pass's last synchronisation for this view)
        finally:
            if release is not None:
                release()
        best = 0
        if np.isfinite(losses[0]):
            for k, l in enumerate(losses):
                if np.isfinite(l) and l < losses[best]:   # strictly smaller: the smallest index wins ties
                    best = k
        pose = poses[best]
        dt, dr = pose_difference(pose, T0)
        return dict(pose=pose, losses=losses, best_iteration=best, loss_given=losses[0], loss_aligned=losses[best],
                    translation=dt, rotation_deg=float(np.degrees(dr)))
