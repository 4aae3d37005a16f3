"""Per-view bilateral grids of affine colour transforms while training.

One affine colour transform per view (exposure.py) absorbs what a photo's exposure and white balance do to the whole frame.  What
varies WITHIN a photo — vignetting, local tone mapping, a white balance that differs between the sunlit and the shaded half — needs
a transform per place and brightness: every training view gets a small grid G [12, L, Gh, Gw] of 3x4 transforms (the identity
[I | 0] in every cell at the start), sliced per pixel by position and luminance and applied to the render before the loss, and
regularised by total variation (BilaRF).  `BilateralGrids` holds the views' grids and their Adam state and never leaves the device:

    batch = grids.begin(view, batch)                    # batch.bilateral_grid = params[view], a VIEW of the state
    stepper.step(batch)                                 # leaves stepper.bilateral_gradient [12,L,Gh,Gw] on the device
    grids.end(view, stepper.bilateral_gradient)         # Adam on that view's floats, in place (gut_bilateral_adam_step)

    rgba2 = grids.apply(view, rgba, background)         # the slice under autograd: the graph reaches the image and the grid

State, all on the device: `params` [V,12,L,Gh,Gw], the Adam moments `m`, `v` of the same shape and the per-view visit counts [V].
Adam runs PER VIEW: a view's moments advance only on its own visits and the bias correction uses the view's own count.  The adjoint
sums integers (§13, §14, §17, §20): identical inputs give identical bits.  Nothing is copied to the host and nothing waits.

Held-out views have no grid and are scored uncorrected: compare runs with and without grids by the colour-corrected metrics
(--cc-metrics).  Data-parallel training with grids does not exist (ValueError in NativeTrainStep).
"""
import copy
import ctypes as C

import numpy as np
import torch

from .confblock import boolean, check_block, integer, number

MAX_DIM = 256   # _capi.BILATERAL_MAX_DIM
# gsplat's published settings for its bilateral grids; UNTUNED here
DEFAULTS = {"enabled": False, "grid": [16, 16, 8], "lr": 0.002, "lambda_tv": 10.0, "start_iteration": 0, "end_iteration": -1,
            "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}
_RATE, _BETA = number("finite and >= 0", ge=0), number("in [0, 1)", ge=0, lt=1)


def _grid_ok(v):
    return isinstance(v, (list, tuple)) and len(v) == 3 and all(isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= MAX_DIM for n in v)


RULES = {"enabled": boolean(), "grid": (_grid_ok, f"three integers [Gw, Gh, L] in 1 .. {MAX_DIM}"), "lr": _RATE, "lambda_tv": _RATE,
         "start_iteration": integer(), "end_iteration": integer(), "eps": _RATE, "beta1": _BETA, "beta2": _BETA}


def check_config(block):
    """The resolved `bilateral` block: grid three integers [Gw, Gh, L] in 1 .. 256, rate, lambda_tv and eps finite and >= 0, betas
    in [0, 1), iterations integers (end_iteration -1: to the end of the run)."""
    check_block("bilateral", block, DEFAULTS, RULES)
    if int(block["start_iteration"]) < 0 or int(block["end_iteration"]) < -1:
        raise ValueError("bilateral: start_iteration must be >= 0 and end_iteration >= 0, or -1 for the end of the run")
    return block


def _plane(t, H, W, channels, name, device):
    if t.dtype != torch.float32 or t.device != device or tuple(t.shape[-3:]) != (H, W, channels) or t.numel() != H * W * channels:
        raise ValueError(f"BilateralGrids: {name} must be a float32 [{H},{W},{channels}] tensor on {device}, got {tuple(t.shape)} "
                         f"{t.dtype} on {t.device}")
    return t.contiguous()


def _background_operand(background, H, W, device):
    """(plane or None, constant) of a background given as a number or as an [H,W,3] / [1,H,W,3] tensor."""
    if isinstance(background, torch.Tensor):
        return _plane(background.detach(), H, W, 3, "background", device), 0.0
    return None, float(background)


def _record(grid):
    from . import _capi
    L, Gh, Gw = (int(n) for n in grid.shape[-3:])
    return _capi.GutBilateralGrid(grid.data_ptr(), L, Gh, Gw)


def workspace_for(lib, grid, workspace=None):
    """An int64 device tensor of at least gut_bilateral_workspace_bytes for `grid` [12,L,Gh,Gw]: `workspace` where it is large enough."""
    L, Gh, Gw = (int(n) for n in grid.shape[-3:])
    need = (lib.gut_bilateral_workspace_bytes(L, Gh, Gw) + 7) // 8
    if need == 0:
        raise ValueError(f"bilateral: grid dimensions must be 1 .. {MAX_DIM}, got {(L, Gh, Gw)} (levels, rows, columns)")
    if workspace is None or workspace.numel() < need or workspace.device != grid.device:
        workspace = torch.empty((need,), dtype=torch.int64, device=grid.device)
    return workspace


def slice_call(lib, H, W, rgba, bg, grid, out):
    """The C call gut_bilateral_slice, nothing checked: contiguous float32 device tensors, rgba and out [H,W,4], grid [12,L,Gh,Gw], bg
    a float or a float32 [H,W,3] device plane.  NativeTrainStep calls this directly, on buffers it sized itself."""
    from . import _capi
    plane = isinstance(bg, torch.Tensor)
    rec = _record(grid)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = lib.gut_bilateral_slice(C.c_void_p(stream), H, W, rgba.data_ptr(), bg.data_ptr() if plane else None, 0.0 if plane else float(bg),
                                     C.byref(rec), out.data_ptr())
    _capi.check(rc, "bilateral_slice")
    return out


def backward_call(lib, H, W, rgba, bg, grid, out_grad, lambda_tv, workspace, rgba_grad, grid_grad):
    """The C call gut_bilateral_backward, nothing checked: operands as slice_call; out_grad and rgba_grad [H,W,4], grid_grad like grid,
    workspace of workspace_for.  Returns (rgba_grad, grid_grad), every element of both written."""
    from . import _capi
    plane = isinstance(bg, torch.Tensor)
    rec = _record(grid)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = lib.gut_bilateral_backward(C.c_void_p(stream), H, W, rgba.data_ptr(), bg.data_ptr() if plane else None,
                                        0.0 if plane else float(bg), C.byref(rec), out_grad.data_ptr(), float(lambda_tv),
                                        workspace.data_ptr(), rgba_grad.data_ptr(), grid_grad.data_ptr())
    _capi.check(rc, "bilateral_backward")
    return rgba_grad, grid_grad


def backward_image_call(lib, H, W, rgba, bg, grid, out_grad, rgba_grad):
    """The C call gut_bilateral_backward_image, nothing checked: backward_call's rgba_grad alone, the same bits, one launch; nothing
    is summed for the grid and no workspace is needed."""
    from . import _capi
    plane = isinstance(bg, torch.Tensor)
    rec = _record(grid)
    stream = torch.cuda.current_stream(rgba.device).cuda_stream
    with torch.cuda.device(rgba.device):
        rc = lib.gut_bilateral_backward_image(C.c_void_p(stream), H, W, rgba.data_ptr(), bg.data_ptr() if plane else None,
                                              0.0 if plane else float(bg), C.byref(rec), out_grad.data_ptr(), rgba_grad.data_ptr())
    _capi.check(rc, "bilateral_backward_image")
    return rgba_grad


class _Slice(torch.autograd.Function):
    """rgba' = slice(rgba, grid): the graph reaches the image and the grid; the backward is gut_bilateral_backward."""

    @staticmethod
    def forward(ctx, rgba, grid, grids, plane, constant):
        ctx.grids, ctx.plane, ctx.constant = grids, plane, constant
        ctx.save_for_backward(rgba, grid)
        return grids._slice(rgba, plane, constant, grid, torch.empty_like(rgba))

    @staticmethod
    def backward(ctx, out_grad):
        rgba, grid = ctx.saved_tensors
        rgba_grad, grid_grad = torch.empty_like(rgba), torch.empty_like(grid)
        ctx.grids._backward(rgba, ctx.plane, ctx.constant, grid, out_grad.contiguous(), 0.0, rgba_grad, grid_grad)
        return rgba_grad, grid_grad, None, None, None


class BilateralGrids:
    def __init__(self, num_views, shape=(16, 16, 8), device="cuda", lr=DEFAULTS["lr"], betas=(0.9, 0.999), eps=1e-15,
                 lambda_tv=DEFAULTS["lambda_tv"], start_iteration=0, end_iteration=-1):
        """num_views: the number of training views; shape: (Gw, Gh, L); device: where the state lives (the stepper's)."""
        V = int(num_views)
        if V <= 0:
            raise ValueError("BilateralGrids: no views")
        if not _grid_ok(list(shape)):
            raise ValueError(f"BilateralGrids: shape must be three integers (Gw, Gh, L) in 1 .. {MAX_DIM}, got {shape!r}")
        Gw, Gh, L = (int(n) for n in shape)
        self.device = torch.device(device)
        self.shape = (Gw, Gh, L)
        identity = torch.zeros((12, L, Gh, Gw), dtype=torch.float32)
        identity[0], identity[5], identity[10] = 1.0, 1.0, 1.0
        self.params = identity.to(self.device).repeat(V, 1, 1, 1, 1).contiguous()
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.counts = torch.zeros((V,), dtype=torch.int32, device=self.device)
        self.lr, self.lambda_tv = float(lr), float(lambda_tv)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError(f"BilateralGrids: betas must be in [0, 1), got {betas!r}")
        if not (0.0 <= self.lambda_tv < float("inf")):
            raise ValueError(f"BilateralGrids: lambda_tv must be finite and >= 0, got {lambda_tv!r}")
        self.start_iteration, self.end_iteration = int(start_iteration), int(end_iteration)
        self._lib, self._workspace = None, None
        if self.device.type == "cuda":
            from . import _capi
            self._lib = _capi.load()
            self._workspace = workspace_for(self._lib, self.params[0])

    @property
    def num_views(self):
        return self.params.shape[0]

    def active(self, step):
        """Whether iteration `step` updates the grids (start_iteration <= step < end_iteration; end_iteration < 0: no end).  Outside,
        the grid is still applied and nothing is scattered or stepped."""
        return step >= self.start_iteration and (self.end_iteration < 0 or step < self.end_iteration)

    def begin(self, view, batch):
        """A shallow copy of `batch` whose `bilateral_grid` is grid `view` of `params` ([12,L,Gh,Gw], a view: the kernels read the
        very floats the view's last end() wrote), and whose `bilateral_lambda_tv` is this object's weight of the TV term."""
        out = copy.copy(batch)
        out.bilateral_grid = self.params[view]
        out.bilateral_lambda_tv = self.lambda_tv
        return out

    # ---- the kernels ----
    def _check_grid(self, grid):
        if grid.dtype != torch.float32 or grid.device != self.device or grid.dim() != 4 or grid.shape[0] != 12 or not grid.is_contiguous():
            raise ValueError(f"BilateralGrids: a grid must be a contiguous float32 [12,L,Gh,Gw] tensor on {self.device}, got "
                             f"{tuple(grid.shape)} {grid.dtype} on {grid.device}")
        if self._lib is None:
            raise RuntimeError("BilateralGrids: the grids are sliced by the HIP library; these live on the host")

    def _slice(self, rgba, plane, constant, grid, out):
        self._check_grid(grid)
        return slice_call(self._lib, int(rgba.shape[-3]), int(rgba.shape[-2]), rgba, constant if plane is None else plane, grid, out)

    def _backward(self, rgba, plane, constant, grid, out_grad, lambda_tv, rgba_grad, grid_grad):
        self._check_grid(grid)
        self._workspace = workspace_for(self._lib, grid, self._workspace)
        return backward_call(self._lib, int(rgba.shape[-3]), int(rgba.shape[-2]), rgba, constant if plane is None else plane, grid, out_grad,
                             lambda_tv, self._workspace, rgba_grad, grid_grad)

    def _operands(self, view_or_grid, rgba, background):
        grid = view_or_grid if isinstance(view_or_grid, torch.Tensor) else self.params[int(view_or_grid)]
        if rgba.shape[-1] != 4 or rgba.dim() not in (3, 4) or (rgba.dim() == 4 and rgba.shape[0] != 1):
            raise ValueError(f"BilateralGrids: rgba must be [H,W,4] or [1,H,W,4], got {tuple(rgba.shape)}")
        H, W = int(rgba.shape[-3]), int(rgba.shape[-2])
        return grid, H, W

    # ---- the public surface ----
    def slice(self, view_or_grid, rgba, background=0.0, out=None):
        """rgba' of rgba [H,W,4] / [1,H,W,4] over `background` (a number, or an [H,W,3] plane) through the view's grid (or a given
        [12,L,Gh,Gw] tensor): gut_bilateral_slice, no graph.  out: a tensor like rgba to write into."""
        grid, H, W = self._operands(view_or_grid, rgba, background)
        rgba = _plane(rgba.detach(), H, W, 4, "rgba", self.device)
        plane, constant = _background_operand(background, H, W, self.device)
        return self._slice(rgba, plane, constant, grid.detach(), torch.empty_like(rgba) if out is None else out)

    def backward(self, view_or_grid, rgba, background, out_grad, rgba_grad=None, grid_grad=None, lambda_tv=None):
        """(rgba_grad, grid_grad) of the slice from out_grad [H,W,4], the gradient a loss wrote for rgba' (gut_bilateral_backward:
        every element of both is written; lambda_tv None: this object's).  No graph."""
        grid, H, W = self._operands(view_or_grid, rgba, background)
        rgba = _plane(rgba.detach(), H, W, 4, "rgba", self.device)
        out_grad = _plane(out_grad.detach(), H, W, 4, "out_grad", self.device)
        plane, constant = _background_operand(background, H, W, self.device)
        rgba_grad = torch.empty_like(rgba) if rgba_grad is None else rgba_grad
        grid_grad = torch.empty_like(grid) if grid_grad is None else grid_grad
        return self._backward(rgba, plane, constant, grid.detach(), out_grad, self.lambda_tv if lambda_tv is None else lambda_tv,
                              rgba_grad, grid_grad)

    def backward_image(self, view_or_grid, rgba, background, out_grad, rgba_grad=None):
        """backward()'s rgba_grad alone, the same bits (gut_bilateral_backward_image): one launch, nothing summed for the grid."""
        grid, H, W = self._operands(view_or_grid, rgba, background)
        rgba = _plane(rgba.detach(), H, W, 4, "rgba", self.device)
        out_grad = _plane(out_grad.detach(), H, W, 4, "out_grad", self.device)
        plane, constant = _background_operand(background, H, W, self.device)
        self._check_grid(grid.detach())
        return backward_image_call(self._lib, H, W, rgba, constant if plane is None else plane, grid.detach(), out_grad,
                                   torch.empty_like(rgba) if rgba_grad is None else rgba_grad)

    def apply(self, view_or_grid, rgba, background=0.0):
        """rgba' = (out, alpha) of rgba over `background` through the view's grid (or a given [12,L,Gh,Gw] tensor).  On the device the
        two kernels under a torch.autograd.Function: the graph reaches the image and the grid (the TV term is not part of it; add
        losses.bilateral_total_variation where it is wanted).  Host tensors go through losses.bilateral_slice, the definition."""
        grid, H, W = self._operands(view_or_grid, rgba, background)
        if self._lib is None or not rgba.is_cuda:
            from .losses import bilateral_slice
            B = background if isinstance(background, torch.Tensor) else float(background)
            comp = rgba[..., 0:3] + B * (1.0 - rgba[..., 3:4])
            return torch.cat([bilateral_slice(comp, grid.to(comp.dtype)), rgba[..., 3:4]], dim=-1)
        plane, constant = _background_operand(background, H, W, self.device)
        rgba = rgba if rgba.is_contiguous() else rgba.contiguous()
        if rgba.dtype != torch.float32 or rgba.device != self.device:
            raise ValueError(f"BilateralGrids.apply: rgba must be float32 on {self.device}, got {rgba.dtype} on {rgba.device}")
        if torch.is_grad_enabled() and (rgba.requires_grad or grid.requires_grad):
            return _Slice.apply(rgba, grid, self, plane, constant)
        return self._slice(rgba, plane, constant, grid.detach(), torch.empty_like(rgba))

    def end(self, view, grid_grad):
        """One Adam step of `view` from grid_grad = d(loss)/dG of its step ([12,L,Gh,Gw], the TV term included by the adjoint), on
        grid_grad's device and stream."""
        p, m, v, cnt = self.params[view], self.m[view], self.v[view], self.counts[view:view + 1]
        if grid_grad.device != self.params.device:
            raise ValueError(f"BilateralGrids.end: the gradient is on {grid_grad.device}, the state on {self.params.device}")
        if grid_grad.numel() != p.numel() or grid_grad.dtype != torch.float32:
            raise ValueError(f"BilateralGrids.end: expected {p.numel()} float32 values, got {tuple(grid_grad.shape)} {grid_grad.dtype}")
        if self._lib is not None:
            from . import _capi
            grid_grad = grid_grad.contiguous()
            stream = torch.cuda.current_stream(grid_grad.device)
            with torch.cuda.device(grid_grad.device):
                rc = self._lib.gut_bilateral_adam_step(C.c_void_p(stream.cuda_stream), grid_grad.data_ptr(), p.data_ptr(), m.data_ptr(),
                                                       v.data_ptr(), cnt.data_ptr(), p.numel(), self.lr, self.betas[0], self.betas[1],
                                                       self.eps)
            _capi.check(rc, "bilateral_adam_step")
        else:
            # host tensors (a stepper without a GPU, in tests): the kernel's arithmetic in float32, as ExposureCompensation.end
            b1, b2 = float(np.float32(self.betas[0])), float(np.float32(self.betas[1]))
            c1, c2 = float(np.float32(1) - np.float32(self.betas[0])), float(np.float32(1) - np.float32(self.betas[1]))
            g = grid_grad.reshape(p.shape).to(torch.float32)
            cnt += 1
            t = int(cnt[0])
            m.mul_(b1).add_(g, alpha=c1)
            v.mul_(b2).add_((g * c2) * g)
            k1, k2 = float(np.float32(1.0 - b1 ** t)), float(np.float32(1.0 - b2 ** t))
            p.sub_((self.lr * (m / k1)) / ((v / k2).sqrt() + self.eps))

    def grids(self):
        """[V,12,L,Gh,Gw] float32 host tensor of the current grids."""
        return self.params.detach().cpu().clone()

    def summary(self):
        """dict(grid, mean_tv, mean_gain): the shape [Gw, Gh, L], the mean TV(G) over the views and the mean of the three diagonal
        channels (reads the state back: end of run)."""
        from .losses import bilateral_total_variation
        G = self.grids().to(torch.float64)
        return dict(grid=list(self.shape), mean_tv=float(bilateral_total_variation(G).mean()), mean_gain=float(G[:, (0, 5, 10)].mean()))

    def state_dict(self):
        """Tensors only (a checkpoint's `native` block must load with weights_only=True): params, moments [V,12,L,Gh,Gw], counts [V]."""
        return dict(params=self.params.detach().cpu().clone(), exp_avg=self.m.detach().cpu().clone(),
                    exp_avg_sq=self.v.detach().cpu().clone(), counts=self.counts.detach().cpu().clone())

    def load_state_dict(self, state):
        params = state["params"]
        if tuple(params.shape) != tuple(self.params.shape):
            raise ValueError(f"BilateralGrids.load_state_dict: the checkpoint holds grids of shape {tuple(params.shape)}, this run has "
                             f"{tuple(self.params.shape)} (views, 12, L, Gh, Gw)")
        # in place: grids handed out by begin() stay views of the state
        self.params.copy_(params)
        self.m.copy_(state["exp_avg"])
        self.v.copy_(state["exp_avg_sq"])
        self.counts.copy_(state["counts"])
