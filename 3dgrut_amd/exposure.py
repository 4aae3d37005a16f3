"""Per-view exposure compensation while training.

The photos of a real capture differ in exposure and white balance.  Every training view gets an affine colour transform
E = [A | b] (3x4, the identity [I | 0] at the start) that is applied to the rendered image inside the loss
(losses.photometric_loss(..., exposure=E) is the definition, gut_photometric_loss_exposure the fused form), and the loss's
backward leaves d(loss)/dE next to the image gradient.  `ExposureCompensation` holds the views' transforms and their Adam state
and never leaves the device:

    batch = exposures.begin(view, batch)                # batch.exposure = params[view], a VIEW of row `view`
    stepper.step(batch)                                 # leaves stepper.exposure_gradient [12] on the device
    exposures.end(view, stepper.exposure_gradient)      # twelve-float Adam on that row, in place (gut_exposure_adam_step)

State, all on the device: `params` [V,12] (row-major E per view), the Adam moments `m`, `v` [V,12] and the per-view visit counts
[V].  Adam runs PER VIEW: a view's moments advance only on its own visits and the bias correction uses the view's own count.
Nothing is copied to the host and nothing waits: the next visit of the view reads the row the kernel updated, on the same stream.

Held-out views have no learnt transform and are scored with the identity: nothing here touches validation or test batches.
Data-parallel exposure compensation does not exist (ValueError in NativeTrainStep).
"""
import copy
import ctypes as C

import numpy as np
import torch

from .confblock import boolean, check_block, integer, number

DEFAULTS = {"enabled": False, "lr": 0.001, "start_iteration": 0, "end_iteration": -1, "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
_RATE, _BETA = number("finite and >= 0", ge=0), number("in [0, 1)", ge=0, lt=1)
RULES = {"enabled": boolean(), "start_iteration": integer(), "end_iteration": integer(), "lr": _RATE, "eps": _RATE, "beta1": _BETA,
         "beta2": _BETA}


def check_config(block):
    """The resolved `exposure` block: rate and eps finite and >= 0, betas in [0, 1), iterations integers (end_iteration -1: to
    the end of the run)."""
    check_block("exposure", block, DEFAULTS, RULES)
    if int(block["start_iteration"]) < 0 or int(block["end_iteration"]) < -1:
        raise ValueError("exposure: start_iteration must be >= 0 and end_iteration >= 0, or -1 for the end of the run")
    return block


class ExposureCompensation:
    def __init__(self, num_views, device, lr=DEFAULTS["lr"], betas=(0.9, 0.999), eps=1e-15, start_iteration=0, end_iteration=-1):
        """num_views: the number of training views; device: where the state lives (the stepper's)."""
        V = int(num_views)
        if V <= 0:
            raise ValueError("ExposureCompensation: no views")
        self.device = torch.device(device)
        self.params = torch.tensor(IDENTITY, dtype=torch.float32, device=self.device).repeat(V, 1).contiguous()
        self.m = torch.zeros((V, 12), dtype=torch.float32, device=self.device)
        self.v = torch.zeros((V, 12), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros((V,), dtype=torch.int32, device=self.device)
        self.lr = float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError(f"ExposureCompensation: betas must be in [0, 1), got {betas!r}")
        self.start_iteration, self.end_iteration = int(start_iteration), int(end_iteration)
        self._lib = None
        if self.device.type == "cuda":
            from . import _capi
            self._lib = _capi.load()

    @property
    def num_views(self):
        return self.params.shape[0]

    def active(self, step):
        """Whether iteration `step` updates the exposures (start_iteration <= step < end_iteration; end_iteration < 0: no end)."""
        return step >= self.start_iteration and (self.end_iteration < 0 or step < self.end_iteration)

    def begin(self, view, batch):
        """A shallow copy of `batch` whose `exposure` is row `view` of `params` ([12], a view: the kernels read the very floats the
        view's last end() wrote)."""
        out = copy.copy(batch)
        out.exposure = self.params[view]
        return out

    def end(self, view, grad12):
        """One Adam step of `view` from grad12 = d(loss)/dE of its step ([12], laid out like E), on grad12's device and stream."""
        if grad12.device != self.params.device:
            raise ValueError(f"ExposureCompensation.end: the gradient is on {grad12.device}, the state on {self.params.device}")
        if grad12.numel() != 12 or grad12.dtype != torch.float32:
            raise ValueError(f"ExposureCompensation.end: expected 12 float32 values, got {tuple(grad12.shape)} {grad12.dtype}")
        p, m, v, cnt = self.params[view], self.m[view], self.v[view], self.counts[view:view + 1]
        if self._lib is not None:
            grad12 = grad12.reshape(12).contiguous()
            stream = torch.cuda.current_stream(grad12.device)
            with torch.cuda.device(grad12.device):
                rc = self._lib.gut_exposure_adam_step(C.c_void_p(stream.cuda_stream), grad12.data_ptr(), p.data_ptr(), m.data_ptr(),
                                                      v.data_ptr(), cnt.data_ptr(), self.lr, self.betas[0], self.betas[1], self.eps)
            if rc:
                raise RuntimeError(f"[3dgut] exposure_adam_step failed ({rc})")
        else:
            # host tensors (a stepper without a GPU, in tests): the kernel's arithmetic in float32 — the betas and 1 - beta held in
            # float32 (1 - 0.999f is 0.0010000467), 1 - beta^t formed in double from the float32 beta and rounded once
            b1, b2 = float(np.float32(self.betas[0])), float(np.float32(self.betas[1]))
            c1, c2 = float(np.float32(1) - np.float32(self.betas[0])), float(np.float32(1) - np.float32(self.betas[1]))
            g = grad12.reshape(12).to(torch.float32)
            cnt += 1
            t = int(cnt[0])
            m.mul_(b1).add_(g, alpha=c1)
            v.mul_(b2).add_((g * c2) * g)
            k1, k2 = float(np.float32(1.0 - b1 ** t)), float(np.float32(1.0 - b2 ** t))
            p.sub_((self.lr * (m / k1)) / ((v / k2).sqrt() + self.eps))

    def exposures(self):
        """[V,3,4] float32 host tensor of the current transforms."""
        return self.params.detach().cpu().reshape(-1, 3, 4).clone()

    def summary(self):
        """dict(mean_gain, mean_offset): the mean of diag(A) and the mean |b| over the views (reads the state back: end of run)."""
        E = self.exposures()
        return dict(mean_gain=float(torch.diagonal(E[:, :, :3], dim1=1, dim2=2).mean()), mean_offset=float(E[:, :, 3].abs().mean()))

    def state_dict(self):
        """Tensors only (a checkpoint's `native` block must load with weights_only=True): params, moments [V,12], counts [V]."""
        return dict(params=self.params.detach().cpu().clone(), exp_avg=self.m.detach().cpu().clone(),
                    exp_avg_sq=self.v.detach().cpu().clone(), counts=self.counts.detach().cpu().clone())

    def load_state_dict(self, state):
        params = state["params"]
        if tuple(params.shape) != tuple(self.params.shape):
            raise ValueError(f"ExposureCompensation.load_state_dict: the checkpoint holds {tuple(params.shape)[0]} exposures, this run "
                             f"has {self.num_views} training views")
        # in place: rows handed out by begin() stay views of the state
        self.params.copy_(params)
        self.m.copy_(state["exp_avg"])
        self.v.copy_(state["exp_avg_sq"])
        self.counts.copy_(state["counts"])
