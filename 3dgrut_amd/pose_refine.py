"""Camera-pose refinement while training.

Every backward of the native train step can leave the view's pose gradient on the device (SplatRaster.set_pose_gradient: a
reduction of the per-Gaussian gradient rows; pose.pose_gradient_from_rows is its definition).  `PoseRefiner` turns those eight
floats into pose updates without putting a host synchronisation into the training loop:

    batch = refiner.begin(view, batch)      # applies the increment that view's LAST visit produced, hands out the refined pose
    stepper.step(batch)                     # leaves stepper.pose_gradient [8] on the device
    refiner.end(view, stepper.pose_gradient)  # six-float Adam on the device, increment copied to a pinned slot behind an event

State: the views' current camera-to-world matrices on the host in float64; on the device the Adam moments `m`, `v` [V,6] and the
per-view visit counts [V].  Adam runs PER VIEW: a view's moments advance only on its own visits and the bias correction uses the
view's own count (a view seen once in an epoch is not "at step 3000").  The increment (d rho, d phi) is composed on the host in
float64 at the view's next `begin`: c += d rho, R <- exp([d phi]x) R — a world-axis twist about the camera centre, the
parametrisation the gradient is taken in.  With two or more views the event of a view last seen a whole step ago has long
completed, so `begin` does not wait; with ONE view it waits for the step before it, every step.

Rays stay as they are: they are in camera space.  Only views with a single pose (pose_start == pose_end) can be refined; the
backward refuses any other while the gradient output is set.  Data-parallel refinement does not exist (ValueError in
NativeTrainStep).  Held-out views are scored at their given poses unless `pose_alignment` is on
(pose_align.py): nothing here touches validation or test batches.
"""
import copy
import ctypes as C

import numpy as np
import torch

from .confblock import boolean, check_block, integer, number
from .pose import apply_pose_increment, pose_difference

DEFAULTS = {"enabled": False, "lr_translation": 0.001, "lr_rotation": 0.0005, "start_iteration": 0, "end_iteration": -1,
            "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}
_RATE, _BETA = number("finite and >= 0", ge=0), number("in [0, 1)", ge=0, lt=1)
RULES = {"enabled": boolean(), "start_iteration": integer(), "end_iteration": integer(), "lr_translation": _RATE, "lr_rotation": _RATE,
         "eps": _RATE, "beta1": _BETA, "beta2": _BETA}


def check_config(block):
    """The resolved `pose_refinement` block: rates and eps finite and >= 0, betas in [0, 1), iterations integers (end_iteration -1:
    to the end of the run)."""
    check_block("pose_refinement", block, DEFAULTS, RULES)
    if int(block["start_iteration"]) < 0 or int(block["end_iteration"]) < -1:
        raise ValueError("pose_refinement: start_iteration must be >= 0 and end_iteration >= 0, or -1 for the end of the run")
    return block


class PoseRefiner:
    def __init__(self, poses_c2w, device, lr_translation, lr_rotation, betas=(0.9, 0.999), eps=1e-15, start_iteration=0,
                 end_iteration=-1):
        """poses_c2w: [V,4,4] camera-to-world matrices of the training views (any float type; kept in float64); device: where the
        moments live (the stepper's); lr_translation: in world units (the trainer multiplies its setting by the scene extent)."""
        p = np.array([np.asarray(torch.as_tensor(m).detach().cpu().numpy(), np.float64).reshape(4, 4) for m in poses_c2w], np.float64)
        if p.ndim != 3 or p.shape[0] == 0:
            raise ValueError("PoseRefiner: no views")
        self.initial = p.copy()
        self.poses = p
        self.device = torch.device(device)
        V = p.shape[0]
        self.m = torch.zeros((V, 6), dtype=torch.float32, device=self.device)
        self.v = torch.zeros((V, 6), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros((V,), dtype=torch.int32, device=self.device)
        self.lr_translation, self.lr_rotation = float(lr_translation), float(lr_rotation)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.start_iteration, self.end_iteration = int(start_iteration), int(end_iteration)
        cuda = self.device.type == "cuda"
        self._delta = torch.zeros((V, 6), dtype=torch.float32, device=self.device)   # the increments as the device wrote them
        self._slots = torch.zeros((V, 6), dtype=torch.float32)                        # ... and their host copies, one slot per view
        if cuda:
            self._slots = self._slots.pin_memory()
            # the copies go into rows of this tensor: a row that did not count as pinned would make them blocking, silently
            if not (self._slots[0].is_pinned() and self._slots[V - 1].is_pinned()):
                raise RuntimeError("PoseRefiner: the rows of the pinned slot tensor are not reported as pinned memory")
        self._events = [None] * V      # the copy into slot v has landed
        self._pending = [False] * V    # slot v holds an increment that has not been applied yet
        self._lib = None
        if cuda:
            from . import _capi
            self._lib, self._check = _capi.load(), _capi.check

    @property
    def num_views(self):
        return self.poses.shape[0]

    def active(self, step):
        """Whether iteration `step` updates the poses (start_iteration <= step < end_iteration; end_iteration < 0: no end)."""
        return step >= self.start_iteration and (self.end_iteration < 0 or step < self.end_iteration)

    def _apply_pending(self, view):
        if not self._pending[view]:
            return
        ev = self._events[view]
        if ev is not None:
            ev.synchronize()   # V >= 2: completed a whole step ago; V == 1: waits for the step before this one, every step
        self.poses[view] = apply_pose_increment(self.poses[view], self._slots[view].numpy().astype(np.float64))
        self._pending[view] = False

    def begin(self, view, batch):
        """Applies the increment pending for `view`, if any, and returns a copy of `batch` whose T_to_world [1,4,4] is the refined
        pose, as a float32 HOST tensor (the tracer builds its camera on the host anyway; no device read-back)."""
        self._apply_pending(view)
        out = copy.copy(batch)
        out.T_to_world = torch.as_tensor(self.poses[view], dtype=torch.float32).reshape(1, 4, 4)
        return out

    def end(self, view, grad8):
        """One Adam step of `view` from the pose gradient grad8 = {F, M, rows, 0} of its backward (dL/d rho = -F, dL/d phi = -M), on
        grad8's device and stream; the increment is copied into the view's pinned slot behind an event and applied at its next
        begin()."""
        if self._pending[view]:
            raise RuntimeError(f"PoseRefiner.end: view {view} has an increment that no begin() has applied yet")
        if grad8.device != self.m.device:
            raise ValueError(f"PoseRefiner.end: the gradient is on {grad8.device}, the refiner's state on {self.m.device}")
        m, v, cnt, delta = self.m[view], self.v[view], self.counts[view:view + 1], self._delta[view]
        if self._lib is not None:
            stream = torch.cuda.current_stream(grad8.device)
            with torch.cuda.device(grad8.device):
                self._check(self._lib.gut_pose_adam_step(C.c_void_p(stream.cuda_stream), grad8.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                         cnt.data_ptr(), self.lr_translation, self.lr_rotation, self.betas[0],
                                                         self.betas[1], self.eps, delta.data_ptr()), "pose_adam_step")
                self._slots[view].copy_(delta, non_blocking=True)
                ev = self._events[view]
                if ev is None:
                    ev = self._events[view] = torch.cuda.Event()
                ev.record(stream)
        else:
            # host tensors (a stepper without a GPU, in tests): the same arithmetic in float32, the betas and 1 - beta held in
            # float32 as the kernel holds them (1 - 0.999f is 0.0010000467)
            b1, b2 = float(np.float32(self.betas[0])), float(np.float32(self.betas[1]))
            c1, c2 = float(np.float32(1) - np.float32(self.betas[0])), float(np.float32(1) - np.float32(self.betas[1]))
            g = -grad8[:6].to(torch.float32)
            cnt += 1
            t = float(int(cnt[0]))
            m.mul_(b1).add_(g, alpha=c1)
            v.mul_(b2).addcmul_(g, g, value=c2)
            lr = torch.tensor([self.lr_translation] * 3 + [self.lr_rotation] * 3, dtype=torch.float32)
            delta.copy_(-lr * (m / (1.0 - b1 ** t)) / ((v / (1.0 - b2 ** t)).sqrt() + self.eps))
            self._slots[view].copy_(delta)
        self._pending[view] = True

    def flush(self):
        """Applies every pending increment (waits for their copies): the poses are then current."""
        for view in range(self.num_views):
            self._apply_pending(view)

    def refined_poses(self):
        """[V,4,4] float64 tensor of the current camera-to-world matrices (pending increments applied first)."""
        self.flush()
        return torch.as_tensor(self.poses.copy())

    def pose_change(self):
        """Mean change of the poses since construction: dict(mean_translation, mean_rotation_deg)."""
        self.flush()
        d = [pose_difference(a, b) for a, b in zip(self.poses, self.initial)]
        return dict(mean_translation=float(np.mean([x[0] for x in d])), mean_rotation_deg=float(np.degrees(np.mean([x[1] for x in d]))))

    def state_dict(self):
        """Tensors only (a checkpoint's `native` block must load with weights_only=True): current and initial poses [V,4,4] float64,
        moments [V,6], visit counts [V]."""
        self.flush()
        return dict(poses=torch.as_tensor(self.poses.copy()), initial_poses=torch.as_tensor(self.initial.copy()),
                    exp_avg=self.m.detach().cpu().clone(), exp_avg_sq=self.v.detach().cpu().clone(), counts=self.counts.detach().cpu().clone())

    def load_state_dict(self, state):
        poses = state["poses"]
        if tuple(poses.shape) != tuple(self.poses.shape):
            raise ValueError(f"PoseRefiner.load_state_dict: the checkpoint holds {tuple(poses.shape)[0]} poses, this run has {self.num_views} training views")
        self.poses = poses.detach().cpu().to(torch.float64).numpy().copy()
        if "initial_poses" in state:
            self.initial = state["initial_poses"].detach().cpu().to(torch.float64).numpy().copy()
        self.m.copy_(state["exp_avg"])
        self.v.copy_(state["exp_avg_sq"])
        self.counts.copy_(state["counts"])
        self._pending = [False] * self.num_views
