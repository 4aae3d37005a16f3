"""End-to-end trainer: the reference's `python train.py --config-name apps/colmap_3dgut.yaml path=...` (threedgrut/trainer.py:
693-806 `run_train_pass`, 861-886 `run_training`, render.py:137-285 for the test split) composed from this tree's pieces:

    NativeGaussianModel(spatial_order=True)      parameters in the tracer's layouts
    NativeTrainStep(schedule=TrainSchedule)      fused loss, lazy Adam moments, side-stream optimiser, in-kernel densification
                                                 statistics; the position-lr decay and the SH-degree ramp run at the end of step()
    GSStrategy(...).attach() / MCMCStrategy      densify / prune / reset / decay, or relocate / add / perturb
    evaluate()                                   held-out PSNR / SSIM on the GPU (gut_image_metrics)

`conf` is a plain dict with the reference's key names; what it leaves out comes from configs/base_gs.yaml + strategy/gs.yaml, or
base_mcmc.yaml + strategy/mcmc.yaml for `strategy.method == "MCMCStrategy"` (`default_config`).  The loop adds no host
synchronisation between events: the loss is read back only when a validation runs.  Views with a mask (`<image stem>_mask.png` next
to the image, io_colmap.ColmapScene.load_mask) train through the masked form of the fused loss; evaluation scores the full image.
`model.background.color: random` composites every training pixel over its own uniform colour, drawn once per step and handed to the
fused loss as a plane (model/background.py:83-89); evaluation scores such a model over black.

Checkpoints hold the reference's get_model_parameters() keys (model/model.py:107-134) with the optimiser state in
torch.optim.Adam.state_dict() layout (six groups, named and ordered as configs/base_gs.yaml), `global_step`, `epoch`, the GS
strategy's densification buffers as 1-tuples (strategy/gs.py:42-48), and one key `native` with what only this trainer needs.
Everything in it is a tensor, number, string, list, tuple or dict: `torch.load(path, weights_only=True)` reads it.  Checkpoints
written by the reference itself (an OmegaConf config inside) are not read.

What is not the reference's is off by default and described where it lives: pose refinement and exposure compensation at
Trainer._build_refiner / _build_exposure, the colour-corrected and pose-aligned metrics at _evaluation_options, densification by
rendering error at _score_error, and the stages that follow train() — STAGES, in run()'s order — at their methods.  Those stages and
the error criterion walk the per-pixel lists, which exist for the unsorted variant at kernel degree 2 only: resolve_config refuses
them elsewhere (require_walk), the Trainer refuses them on several GPUs (require_one_gpu).  FLAGS is the command line.

    python -m 3dgrut_amd.trainer --path DIR [--out-dir D] [--n-iterations N] [--strategy gs|mcmc] [--downsample F]
                                 [--test-split-interval 8] [--resume CKPT] [--background black|white|random]
                                 [--refine-poses [--pose-lr-translation X] [--pose-lr-rotation R]]
                                 [--exposure [--exposure-lr X]] [--cc-metrics] [--aligned-metrics [--align-iterations K]]
                                 [--compact-to FRACTION [--compact-score weight_sum|max_weight] [--compact-finetune K]]
                                 [--densify-by gradient|error [--densify-grow-fraction F] [--densify-views K]]
                                 [--select-by-masks [SUFFIX] [--select-threshold T]]
                                 [--fit-features [SUFFIX] [--feature-iterations K] [--feature-lr X]]
                                 [--export-points [--points-level T] [--points-stride S] [--points-voxel V]]
                                 [--export-mesh [--mesh-resolution R] [--mesh-voxel V]]
                                 [--environment [--environment-resolution R] [--environment-lr X]]
                                 [--bilateral [--bilateral-grid X Y L] [--bilateral-lr X] [--bilateral-tv X]]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

from . import contribution as contribution_mod
from . import features as features_mod
from . import bilateral as bilateral_mod
from . import environment as environment_mod
from . import exposure as exposure_mod
from . import losses, pose_align, pose_refine
from . import mesh as mesh_mod
from . import selection as selection_mod
from . import surface as surface_mod
from .confblock import boolean, check_block, integer, nullable, number, one_of
from .evaluate import _check_batch, evaluate
from .strategy import CRITERIA, ERROR_SCORES

# configs/base_gs.yaml + configs/strategy/gs.yaml: the keys this trainer reads
GS_CONFIG = {
    "out_dir": "./runs", "resume": "", "n_iterations": 30000, "val_frequency": 5000, "validate_first": False, "test_last": True,
    "seed": 0,
    "checkpoint": {"iterations": [7000, 30000]},
    "model": {"default_density": 0.1, "default_scale_factor": 1.0,
              "progressive_training": {"feature_type": "sh", "init_n_features": 0, "max_n_features": 3, "increase_frequency": 1000,
                                       "increase_step": 1},
              "background": {"name": "background-color", "color": "black"}},
    "optimizer": {"type": "adam", "eps": 1e-15,
                  "params": {"positions": {"lr": 0.00016}, "density": {"lr": 0.05}, "features_albedo": {"lr": 0.0025},
                             "features_specular": {"lr": 0.0025 / 20}, "rotation": {"lr": 0.001}, "scale": {"lr": 0.005}}},
    "scheduler": {"positions": {"type": "exp", "lr_final": 0.0000016, "max_steps": 30000}},
    "loss": {"use_l1": True, "lambda_l1": 0.8, "use_l2": False, "lambda_l2": 1.0, "use_ssim": True, "lambda_ssim": 0.2,
             "use_opacity": False, "lambda_opacity": 0.0, "use_scale": False, "lambda_scale": 0.0},
    "render": {"enable_kernel_timings": False},
    # not a reference key: camera-pose refinement of the training views (pose_refine.py).  lr_translation is multiplied by the scene
    # extent, lr_rotation is in radians; end_iteration -1 = to the end of the run.  The two rates are untuned on real captures.
    "pose_refinement": dict(pose_refine.DEFAULTS),
    # not a reference key: a learnt affine colour transform per training view (exposure.py).  end_iteration -1 = to the end of the run.
    # The rate is untuned on real captures.
    "exposure": dict(exposure_mod.DEFAULTS),
    # not a reference key: colour-corrected held-out metrics next to the plain ones (evaluate.py).  ridge is the regulariser of the
    # per-view affine fit, a parameter of the metric's definition (> 0), not a tolerance.
    "evaluation": {"colour_corrected": False, "ridge": 1e-6},
    # not a reference key: pose-aligned held-out metrics next to the plain ones (pose_align.py).  lr_translation is multiplied by the
    # scene extent, lr_rotation is in radians; validation: the validation passes too, not only the final test pass.  The two rates and
    # the iteration count are untuned on real captures.
    "pose_alignment": dict(pose_align.DEFAULTS),
    # not reference keys: the stages that follow train() (STAGES; each block is described at its Trainer method)
    "compaction": dict(contribution_mod.DEFAULTS), "selection": dict(selection_mod.DEFAULTS), "features": dict(features_mod.DEFAULTS),
    "points": dict(surface_mod.DEFAULTS), "mesh": dict(mesh_mod.DEFAULTS),
    "strategy": {"method": "GSStrategy",
                 # criterion and error are not reference keys: "error" grows, at every densify step, the grow_fraction of the rows
                 # that are responsible for the most rendering error over `views` training views (0: all of them), instead of
                 # thresholding the position-gradient statistics (strategy.select_by_error).  grow_fraction, views
                 # and min_pixels are untuned on real captures.
                 "densify": {"frequency": 300, "start_iteration": 500, "end_iteration": 15000, "clone_grad_threshold": 0.0002,
                             "split_grad_threshold": 0.0002, "relative_size_threshold": 0.01, "split": {"n_gaussians": 2},
                             "criterion": "gradient",
                             "error": {"grow_fraction": 0.05, "score": "error_sum", "min_pixels": 1, "views": 0, "max_n_gaussians": None}},
                 "prune": {"frequency": 100, "start_iteration": 500, "end_iteration": 15000, "density_threshold": 0.005},
                 # end_iteration None: ${strategy.densify.end_iteration}, as the yaml interpolates it
                 "reset_density": {"frequency": 3000, "start_iteration": 0, "end_iteration": None, "new_max_density": 0.01},
                 "density_decay": {"gamma": 0.99, "start_iteration": -1, "end_iteration": -1, "frequency": 50}},
}
# configs/base_mcmc.yaml + configs/strategy/mcmc.yaml over GS_CONFIG
MCMC_OVERRIDES = {
    "model": {"default_density": 0.5, "default_scale_factor": 0.1},
    "loss": {"use_opacity": True, "lambda_opacity": 0.01, "use_scale": True, "lambda_scale": 0.01},
    "strategy": {"method": "MCMCStrategy", "binom_n_max": 51, "opacity_threshold": 0.005,
                 "relocate": {"start_iteration": 500, "end_iteration": 25000, "frequency": 100},
                 "perturb": {"start_iteration": 0, "end_iteration": 27500, "frequency": 1, "noise_lr": 500000.0},
                 "add": {"start_iteration": 500, "end_iteration": 25000, "frequency": 100, "max_n_gaussians": 1000000}},
}
# the reference's optimiser groups, in configs/base_gs.yaml order, and where each lives in the native tensors
PARAM_GROUPS = ("positions", "density", "features_albedo", "features_specular", "rotation", "scale")
_GROUP_COLS = {"positions": ("12", slice(0, 3)), "density": ("12", slice(3, 4)), "rotation": ("12", slice(4, 8)),
               "scale": ("12", slice(8, 11)), "features_albedo": ("48", slice(0, 3)), "features_specular": ("48", slice(3, 48))}


def _merge(base, over):
    """Deep merge of plain dicts: `over` wins, nested dicts are merged key by key."""
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


def default_config(method="GSStrategy"):
    """The reference's defaults for `method` ("GSStrategy" or "MCMCStrategy") as a plain dict."""
    if method == "GSStrategy":
        return copy.deepcopy(GS_CONFIG)
    if method == "MCMCStrategy":
        base = copy.deepcopy(GS_CONFIG)
        base["strategy"] = {}
        return _merge(base, MCMC_OVERRIDES)
    raise ValueError(f"unknown strategy.method {method!r} (GSStrategy or MCMCStrategy)")


def resolve_config(conf):
    """conf (a plain dict, any subset of the reference's keys) over the defaults of its strategy.method."""
    conf = dict(conf or {})
    method = (conf.get("strategy") or {}).get("method", "GSStrategy")
    out = _merge(default_config(method), conf)
    if method == "GSStrategy" and out["strategy"]["reset_density"].get("end_iteration") is None:
        out["strategy"]["reset_density"]["end_iteration"] = out["strategy"]["densify"]["end_iteration"]
    pose_refine.check_config(out["pose_refinement"])
    exposure_mod.check_config(out["exposure"])
    # not a reference key, and not among the defaults above: a learnt cube-map background behind the Gaussians (environment.py,
    # DESIGN.md §20), resolved here over its own defaults.  end_iteration null = to the end of the run; outside the window the map
    # is still composited.  lr, init and resolution are untuned on real captures.
    out["environment"] = _merge(environment_mod.DEFAULTS, out.get("environment"))
    check_environment_config(out)
    # likewise: a learnt bilateral grid of affine colour transforms per training view (bilateral.py), resolved over
    # its own defaults (gsplat's published settings, untuned here).  end_iteration -1 = to the end of the run; outside the window
    # the grids are still applied.
    out["bilateral"] = _merge(bilateral_mod.DEFAULTS, out.get("bilateral"))
    check_bilateral_config(out)
    check_evaluation_config(out["evaluation"])
    pose_align.check_config(out["pose_alignment"])
    contribution_mod.check_config(out["compaction"])
    selection_mod.check_config(out["selection"])
    features_mod.check_config(out["features"])
    surface_mod.check_config(out["points"])
    mesh_mod.check_config(out["mesh"])
    for block, _, noun, walks in STAGES:      # (a disabled stage is never refused)
        if walks and out[block]["enabled"]:
            require_walk(out, f"{block}: the {noun}")
    check_densify_config(out)
    if "features_specular" not in ((conf.get("optimizer") or {}).get("params") or {}):
        # ${div:${optimizer.params.features_albedo.lr},20}
        out["optimizer"]["params"]["features_specular"] = {"lr": float(out["optimizer"]["params"]["features_albedo"]["lr"]) / 20}
    return out


# the stages that follow train(), in the order run() walks them: (conf block, Trainer method, the noun of its refusals, whether it
# walks the per-pixel lists)
STAGES = (("compaction", "compact", "compaction", True), ("selection", "select_by_masks", "selection", True),
          ("features", "fit_features", "feature fitting", True), ("points", "export_points", "point export", True),
          ("mesh", "export_mesh", "mesh export", True))


def require_walk(conf, who):
    """`who` (the subject of the refusal) needs one of the per-pixel walks — contribution, attributes, surface — which exist for the
    unsorted variant (render.splat.k_buffer_size 0) at kernel degree 2 only."""
    render = conf.get("render") or {}
    k_buffer = int((render.get("splat") or {}).get("k_buffer_size", 0))
    degree = int(render.get("particle_kernel_degree", 2))
    if k_buffer > 0:
        raise ValueError(f"{who} needs the unsorted variant (render.splat.k_buffer_size is {k_buffer})")
    if degree != 2:
        raise ValueError(f"{who} needs render.particle_kernel_degree 2 (it is {degree})")


def require_one_gpu(stepper, block, noun):
    """None of what this trainer adds to the reference exists data-parallel."""
    if int(getattr(stepper, "world_size", 1)) > 1:
        raise ValueError(f"{block}: data-parallel {noun} is out of scope (the stepper's world_size must be 1)")


DENSIFY_ERROR_DEFAULTS = GS_CONFIG["strategy"]["densify"]["error"]
DENSIFY_ERROR_RULES = {"grow_fraction": number("in (0, 1]", gt=0, le=1), "score": one_of(ERROR_SCORES), "min_pixels": integer(ge=0),
                       "views": integer(ge=0), "max_n_gaussians": nullable(integer(ge=1))}
EVALUATION_RULES = {"colour_corrected": boolean(), "ridge": number("finite and > 0", gt=0)}


def check_densify_config(conf):
    """strategy.densify.criterion and strategy.densify.error of a resolved conf.  criterion "error" is for GSStrategy, and where the
    weighted contribution walk exists (require_walk); the data-parallel refusal needs the stepper and is the Trainer's."""
    densify = conf["strategy"].get("densify") or {}
    criterion = densify.get("criterion", "gradient")
    if criterion not in CRITERIA:
        raise ValueError(f"strategy.densify.criterion must be one of {CRITERIA}, got {criterion!r}")
    if conf["strategy"]["method"] != "GSStrategy":
        if criterion != "gradient":
            raise ValueError(f"strategy.densify.criterion: {criterion!r} is for GSStrategy only (MCMC sampling by error is out of scope)")
        return conf
    check_block("strategy.densify.error", densify["error"], DENSIFY_ERROR_DEFAULTS, DENSIFY_ERROR_RULES)
    if criterion == "error":
        require_walk(conf, "strategy.densify.criterion: 'error'")
        if int(densify["split"]["n_gaussians"]) != 2:
            raise ValueError("strategy.densify.criterion: 'error' grows one row per selected row (strategy.densify.split.n_gaussians must be 2)")
    return conf


def check_environment_config(conf):
    """The `environment` block of a resolved conf, and what an enabled map refuses: another background colour beside it (the map IS
    the background) and pose-aligned metrics (the plane depends on the pose being fitted, and that dependence has no gradient).  The
    data-parallel refusal needs the stepper and is the Trainer's."""
    block = environment_mod.check_config(conf["environment"])
    if block["enabled"]:
        color = conf["model"]["background"]["color"]
        if color != "black":
            raise ValueError(f"environment: the map is the background, model.background.color must be 'black' (it is {color!r})")
        if conf["pose_alignment"]["enabled"]:
            raise ValueError("environment: pose-aligned metrics are refused with an environment map (pose_alignment.enabled): the "
                             "background plane depends on the pose being fitted, and that dependence has no gradient")
    return conf


def check_bilateral_config(conf):
    """The `bilateral` block of a resolved conf, and what enabled grids refuse: exposure compensation beside them (a grid contains the
    global affine, and the two are degenerate against each other).  The data-parallel refusal needs the stepper and is the
    Trainer's."""
    block = bilateral_mod.check_config(conf["bilateral"])
    if block["enabled"] and conf["exposure"]["enabled"]:
        raise ValueError("bilateral: a bilateral grid contains the global affine of exposure.enabled, and the two are degenerate against "
                         "each other; enable one of them")
    return conf


def check_evaluation_config(block):
    """The resolved `evaluation` block: colour_corrected true or false, ridge finite and > 0."""
    return check_block("evaluation", block, GS_CONFIG["evaluation"], EVALUATION_RULES)


# what a pose-aligned evaluation adds to the validation entries and to main()'s final JSON, where the evaluator returned it
PA_SUMMARY_KEYS = ("mean_pa_psnr", "std_pa_psnr", "mean_pa_ssim", "mean_pa_translation", "mean_pa_rotation_deg", "mean_pa_cc_psnr",
                   "std_pa_cc_psnr", "mean_pa_cc_ssim")

BACKGROUND_COLORS = ("black", "white", "random")   # configs/base_gs.yaml:72-74


def check_background_color(conf):
    """model.background.color of a resolved conf must be one the reference's BackgroundColor.setup takes (background.py:66-70)."""
    color = conf["model"]["background"]["color"]
    if color not in BACKGROUND_COLORS:
        raise ValueError(f"Background color must be one of 'white', 'black', 'random' (model.background.color is {color!r})")
    return color


def _stage(t, s):
    """(start, end, frequency) of a strategy block (utils/misc.check_step_condition's arguments)."""
    return (int(t[s]["start_iteration"]), int(t[s]["end_iteration"]), int(t[s]["frequency"]))


def gs_schedule(conf):
    s = conf["strategy"]
    return dict(densify=_stage(s, "densify"), prune=_stage(s, "prune"), reset_density=_stage(s, "reset_density"),
                density_decay=_stage(s, "density_decay"))


def mcmc_schedule(conf):
    s = conf["strategy"]
    return dict(relocate=_stage(s, "relocate"), add=_stage(s, "add"), perturb=_stage(s, "perturb"))


def epoch_permutation(seed, epoch, n):
    """View order of one epoch: a permutation from a torch.Generator seeded with (seed, epoch), so that a resumed run walks the
    same order from the same step on (the reference uses a shuffling DataLoader)."""
    g = torch.Generator().manual_seed(int(seed) * 1_000_003 + int(epoch))
    return torch.randperm(int(n), generator=g).tolist()


def _plain(x):
    """conf -> only dicts, lists, strings, numbers, bools and None (what torch.load(weights_only=True) accepts)."""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, (bool, int, float, str)) or x is None:
        return x
    if isinstance(x, np.generic):
        return x.item()
    return str(x)


def _adam_group_template(betas, eps):
    """The param_groups entry torch.optim.Adam itself would write (every key of the installed torch version)."""
    g = torch.optim.Adam([torch.zeros(1)], lr=1.0, betas=tuple(betas), eps=float(eps)).state_dict()["param_groups"][0]
    g.pop("params")
    return g


def make_checkpoint(stepper, conf, global_step, epoch, scene_extent, strategy=None, refiner=None, exposures=None, environment=None,
                    bilateral=None):
    """The checkpoint dictionary of a NativeTrainStep's state (see the module docstring); refiner: the run's PoseRefiner or None;
    exposures: its ExposureCompensation or None; environment: its EnvironmentMap or None; bilateral: its BilateralGrids or None."""
    from .io_ply import checkpoint_dict
    st = stepper.state_dict()   # moments brought up to date (sync_moments) and cloned
    m = stepper.model
    moments = {("12", 0): st["exp_avg_raw"], ("12", 1): st["exp_avg_sq_raw"], ("48", 0): st["exp_avg_features"],
               ("48", 1): st["exp_avg_sq_features"]}
    lr = {"12": np.asarray(stepper.lr12, np.float32), "48": np.asarray(stepper.lr48, np.float32)}
    tmpl = _adam_group_template(getattr(stepper, "betas", (0.9, 0.999)), getattr(stepper, "eps", 1e-15))
    state, groups = {}, []
    for i, name in enumerate(PARAM_GROUPS):
        block, cols = _GROUP_COLS[name]
        state[i] = {"step": torch.tensor(float(st["step"])), "exp_avg": moments[(block, 0)][:, cols].contiguous(),
                    "exp_avg_sq": moments[(block, 1)][:, cols].contiguous()}
        groups.append(dict(tmpl, lr=float(lr[block][cols.start]), name=name, params=[i]))
    prog = conf["model"]["progressive_training"]
    sched = getattr(stepper, "schedule", None)
    progressive = int(prog["init_n_features"]) < int(prog["max_n_features"])
    color = conf["model"]["background"]["color"]
    extra = {
        # (zeros for `random` as well: BackgroundColor.setup stores black for it, the colour used when not training)
        "background": {"color": torch.full((3,), 1.0 if color == "white" else 0.0, dtype=torch.float32)},
        "progressive_training": progressive, "scene_extent": float(scene_extent), "config": _plain(conf),
        "optimizer": {"state": state, "param_groups": groups}, "global_step": int(global_step), "epoch": int(epoch),
        "native": {"step": int(st["step"]), "lr_raw": torch.as_tensor(lr["12"]).clone(), "lr_features": torch.as_tensor(lr["48"]).clone(),
                   "position_lr": float(sched.position_lr) if sched is not None else float(lr["12"][0]),
                   # column 11 of the raw rows (unused by the kernels) and of their two moments: not a reference parameter
                   "pad": torch.stack([m.raw[:, 11], st["exp_avg_raw"][:, 11], st["exp_avg_sq_raw"][:, 11]], 1).detach().clone(),
                   "permutation": None if getattr(m, "permutation", None) is None else m.permutation.detach().clone(),
                   "spatial_order": bool(getattr(m, "spatial_order", False))},
    }
    if refiner is not None:
        extra["native"]["pose_refinement"] = refiner.state_dict()   # tensors only: poses, moments, visit counts
    if exposures is not None:
        extra["native"]["exposure"] = exposures.state_dict()        # tensors only: transforms, moments, visit counts
    if environment is not None:
        extra["native"]["environment"] = environment.state_dict()   # tensors only: texels, Adam's moments and step count
    if bilateral is not None:
        extra["native"]["bilateral"] = bilateral.state_dict()       # tensors only: grids, moments, visit counts
    if progressive:
        extra["feature_dim_increase_interval"] = int(prog["increase_frequency"])
        extra["feature_dim_increase_step"] = int(prog["increase_step"])
    if strategy is not None and hasattr(strategy, "grad_norm_accum"):
        extra["densify_grad_norm_accum"] = (strategy.grad_norm_accum.detach().clone(),)
        extra["densify_grad_norm_denom"] = (strategy.grad_norm_denom.detach().clone(),)
    return checkpoint_dict(m, extra)


def checkpoint_tensors(ckpt, device):
    """(raw [N,12], features [N,48], optimiser state for NativeTrainStep.load_state_dict) of a checkpoint dictionary."""
    dev = torch.device(device)
    t = lambda x: x.to(dev)
    nat = ckpt["native"]
    pad = t(nat["pad"])
    raw = torch.cat([t(ckpt["positions"]), t(ckpt["density"]), t(ckpt["rotation"]), t(ckpt["scale"]), pad[:, 0:1]], 1).contiguous()
    features = torch.cat([t(ckpt["features_albedo"]), t(ckpt["features_specular"])], 1).contiguous()
    st = ckpt["optimizer"]["state"]
    by_name = {g["name"]: st[g["params"][0]] for g in ckpt["optimizer"]["param_groups"]}
    state = {"step": int(nat["step"]), "lr_raw": nat["lr_raw"].cpu().numpy()}
    for k, key in ((0, "exp_avg"), (1, "exp_avg_sq")):
        raw_m = torch.cat([t(by_name[n][key]) for n in ("positions", "density", "rotation", "scale")] + [pad[:, 1 + k:2 + k]], 1)
        feat_m = torch.cat([t(by_name[n][key]) for n in ("features_albedo", "features_specular")], 1)
        state["exp_avg_raw" if k == 0 else "exp_avg_sq_raw"] = raw_m.contiguous()
        state["exp_avg_features" if k == 0 else "exp_avg_sq_features"] = feat_m.contiguous()
    return raw, features, state


class Trainer:
    """The reference's training run on the native pieces.  `scene`: the initial Gaussians (activated parameters, the dict
    io_colmap.ColmapScene.initial_gaussians / scenes.* return); `*_batches`: protocols.Batch with rgb_gt.  A training batch may carry a
    mask [1,H,W,1]: the stepper multiplies prediction and ground truth by it inside the loss (trainer.py:397-404), so it must say
    `supports_masks = True` (NativeTrainStep and train.TrainStep do) — with one that does not, a masked training batch is a
    ValueError, not a view silently trained on its masked-out pixels.  Masks of validation and test batches are accepted and
    ignored: held-out metrics are of the full image, as in the reference.

    stepper / strategy / evaluator: replacements of the NativeTrainStep, the strategy object and `evaluate` (tests); with a
    stepper given, `scene` is not used and the model is stepper.model."""

    def __init__(self, conf, scene, train_batches, val_batches=(), test_batches=(), scene_extent=1.0, stepper=None, strategy=None,
                 evaluator=None, tracer=None):
        self.conf = resolve_config(conf)
        c = self.conf
        check_background_color(c)
        self.train_batches, self.val_batches, self.test_batches = list(train_batches), list(val_batches), list(test_batches)
        if not self.train_batches:
            raise ValueError("Trainer: no training views")
        for what, bs in (("train", self.train_batches), ("validation", self.val_batches), ("test", self.test_batches)):
            for b in bs:
                _check_batch(b, f"Trainer ({what} batch)")
        # (a stepper built here is a NativeTrainStep, which honours masks)
        if stepper is not None and not getattr(stepper, "supports_masks", False) \
                and any(getattr(b, "mask", None) is not None for b in self.train_batches):
            raise ValueError(f"Trainer (train batch): a batch carries a mask and {type(stepper).__name__} does not honour masks "
                             "(no `supports_masks = True`): it would train on the masked-out pixels")
        self.scene_extent = float(scene_extent)
        self.method = c["strategy"]["method"]
        self.evaluator = evaluate if evaluator is None else evaluator
        self.global_step = 0
        self.validations = []    # dict(step, loss, mean_psnr, ...) per validation pass
        self.stats = None
        self.test_metrics = None
        resume = c.get("resume") or ""
        ckpt = torch.load(resume, map_location="cpu", weights_only=True) if resume else None
        if stepper is None:
            stepper, tracer = self._build(scene, ckpt, tracer)
        self.stepper, self.tracer = stepper, tracer if tracer is not None else getattr(stepper, "tracer", None)
        self.model = stepper.model
        self.strategy = self._build_strategy(ckpt) if strategy is None else strategy
        self.refiner = self._build_refiner(ckpt)
        self.exposure = self._build_exposure(ckpt)
        self.environment_map = self._build_environment(ckpt)
        self.bilateral = self._build_bilateral(ckpt)
        if ckpt is not None:
            self.global_step = int(ckpt["global_step"])
        for block, _, noun, _ in STAGES:
            if c[block]["enabled"]:
                require_one_gpu(stepper, block, noun)
        self.densify_criterion = (c["strategy"].get("densify") or {}).get("criterion", "gradient")
        if self.densify_criterion == "error":
            require_one_gpu(stepper, "strategy.densify.criterion", "error-based densification")
            if getattr(self.strategy, "error_scorer", None) is None:
                self.strategy.error_scorer = self._score_error

    # ---- construction ----
    def _build(self, scene, ckpt, tracer):
        from .native import NativeGaussianModel, NativeTrainStep
        from .schedule import TrainSchedule
        from .tracer import Tracer
        c = self.conf
        prog = c["model"]["progressive_training"]
        if int(prog["max_n_features"]) != 3:
            raise ValueError("Trainer: model.progressive_training.max_n_features must be 3 (the fused optimiser's SH layout)")
        if c["optimizer"]["type"] not in ("adam", "selective_adam"):
            raise ValueError(f"Unknown optimizer type: {c['optimizer']['type']}")
        lr = {k: float(v["lr"]) for k, v in c["optimizer"]["params"].items()}
        sp = c["scheduler"]["positions"]
        sched = TrainSchedule(self.scene_extent, lr_init=lr["positions"], lr_final=float(sp["lr_final"]), max_steps=int(sp["max_steps"]),
                              init_n_features=int(prog["init_n_features"]), max_n_features=int(prog["max_n_features"]),
                              increase_frequency=int(prog["increase_frequency"]), increase_step=int(prog["increase_step"]))
        if tracer is None:
            tracer = Tracer({"render": dict(c.get("render") or {})})
        bg = c["model"]["background"]["color"]
        if ckpt is None:
            model = NativeGaussianModel(scene, sh_degree=sched.n_active_features, background_color=bg, spatial_order=True)
            state = None
        else:
            raw, features, state = checkpoint_tensors(ckpt, "cuda")
            nat = ckpt["native"]
            perm = nat.get("permutation")
            model = NativeGaussianModel.from_tensors(raw, features, sh_degree=int(ckpt["n_active_features"]), background_color=bg,
                                                     spatial_order=bool(nat.get("spatial_order", True)),
                                                     permutation=None if perm is None else perm.to(raw.device))
            sched.position_lr = float(nat["position_lr"])      # the schedule's state: current position rate and SH degree
            sched.n_active_features = int(ckpt["n_active_features"])
        stepper = NativeTrainStep(model, tracer, scene_extent=self.scene_extent, selective=c["optimizer"]["type"] == "selective_adam",
                                  eps=float(c["optimizer"].get("eps", 1e-15)), schedule=sched,
                                  pose_gradient=bool(c["pose_refinement"]["enabled"]),
                                  exposure_gradient=bool(c["exposure"]["enabled"]),
                                  bilateral_gradient=bool(c["bilateral"]["enabled"]), **losses.loss_weights(c["loss"]))
        stepper.lr12[0:3] = sched.position_lr
        stepper.lr12[3] = lr["density"]
        stepper.lr12[4:8] = lr["rotation"]
        stepper.lr12[8:11] = lr["scale"]
        stepper.lr48[0:3] = lr["features_albedo"]
        stepper.lr48[3:] = lr["features_specular"]
        if state is not None:
            stepper.load_state_dict(state)   # moments, step counter (the lazy waves re-based on it), learning rates
        return stepper, tracer

    def _build_refiner(self, ckpt):
        """The PoseRefiner of a run with pose_refinement.enabled (default off; `--refine-poses`), else None; its state restored
        from a resumed checkpoint.  It refines the training views' camera poses while training (pose_refine.PoseRefiner): every
        step's backward leaves the view's pose gradient on the device, a per-view Adam turns it into an increment, and the view's
        next visit renders from the refined pose.  Held-out views (validation, test) are scored at their GIVEN poses unless
        `pose_alignment` is on.  The refiner's poses, moments and visit counts travel in the checkpoint's `native` block as tensors."""
        pr = self.conf["pose_refinement"]
        if not pr["enabled"]:
            if ckpt is not None and ckpt.get("native", {}).get("pose_refinement") is not None:
                # continuing at the GIVEN poses would silently drop the refined ones the Gaussians were trained against
                raise ValueError("pose_refinement: the checkpoint holds refined poses and pose_refinement.enabled is off; resume with "
                                 "--refine-poses (pose_refinement.enabled: true), with end_iteration 0 to keep the poses as they are")
            return None
        st = self.stepper
        require_one_gpu(st, "pose_refinement", "pose refinement")
        if getattr(st, "pose_gradient", None) is None:
            raise ValueError(f"pose_refinement: {type(st).__name__} leaves no pose gradient (NativeTrainStep(..., pose_gradient=True) does)")
        refiner = pose_refine.PoseRefiner([b.T_to_world for b in self.train_batches], st.pose_gradient.device,
                                          lr_translation=float(pr["lr_translation"]) * self.scene_extent, lr_rotation=float(pr["lr_rotation"]),
                                          betas=(float(pr["beta1"]), float(pr["beta2"])), eps=float(pr["eps"]),
                                          start_iteration=int(pr["start_iteration"]), end_iteration=int(pr["end_iteration"]))
        saved = None if ckpt is None else ckpt["native"].get("pose_refinement")
        if saved is not None:
            refiner.load_state_dict(saved)
        return refiner

    def _build_exposure(self, ckpt):
        """The ExposureCompensation of a run with exposure.enabled (default off; `--exposure`), else None; its state restored from a
        resumed checkpoint.  It learns an affine colour transform per training view: the loss compares A image + b
        with the photo, its backward leaves d(loss)/d[A | b] on the device, and a per-view Adam updates the view's twelve floats
        there.  Held-out views have no learnt transform and are scored with the identity.  The transforms, moments and visit counts
        travel in the checkpoint's `native` block as tensors."""
        ex = self.conf["exposure"]
        if not ex["enabled"]:
            if ckpt is not None and ckpt.get("native", {}).get("exposure") is not None:
                # continuing without them would silently drop the transforms the Gaussians were trained against
                raise ValueError("exposure: the checkpoint holds learnt exposures and exposure.enabled is off; resume with --exposure "
                                 "(exposure.enabled: true), with end_iteration 0 to keep the exposures as they are")
            return None
        st = self.stepper
        require_one_gpu(st, "exposure", "exposure compensation")
        if getattr(st, "exposure_gradient", None) is None:
            raise ValueError(f"exposure: {type(st).__name__} leaves no exposure gradient (NativeTrainStep(..., exposure_gradient=True) does)")
        comp = exposure_mod.ExposureCompensation(len(self.train_batches), st.exposure_gradient.device, lr=float(ex["lr"]),
                                                 betas=(float(ex["beta1"]), float(ex["beta2"])), eps=float(ex["eps"]),
                                                 start_iteration=int(ex["start_iteration"]), end_iteration=int(ex["end_iteration"]))
        saved = None if ckpt is None else ckpt["native"].get("exposure")
        if saved is not None:
            comp.load_state_dict(saved)
        return comp

    def _build_environment(self, ckpt):
        """The EnvironmentMap of a run with environment.enabled (default off; `--environment`), else None; its state restored from a
        resumed checkpoint.  It is a learnt radiance at infinity: a cube map [6,R,R,3] composited behind the
        Gaussians in training and at evaluation (model.environment, through background()), so that sky and far background need no
        large faint Gaussians.  Inside [start_iteration, end_iteration) every step scatters (1 - alpha) d loss / d rgb onto the
        texels and takes an Adam step on them, on the device; outside, the map is composited as it is.  With --refine-poses the plane
        is sampled from the refined pose; the pose gradient does not see the map (as it does not see the SH view direction).  The
        texels and their Adam state travel in the checkpoint's `native` block as tensors."""
        blk = self.conf["environment"]
        if not blk["enabled"]:
            if ckpt is not None and ckpt.get("native", {}).get("environment") is not None:
                # continuing over black would silently drop the background the Gaussians were trained against
                raise ValueError("environment: the checkpoint holds an environment map and environment.enabled is off; resume with "
                                 "--environment (environment.enabled: true), with end_iteration 0 to keep the map as it is")
            return None
        st = self.stepper
        require_one_gpu(st, "environment", "environment-map training")
        env = environment_mod.EnvironmentMap(int(blk["resolution"]), float(blk["init"]), self.model.raw.device, lr=float(blk["lr"]),
                                             start_iteration=int(blk["start_iteration"]), end_iteration=blk["end_iteration"])
        saved = None if ckpt is None else ckpt["native"].get("environment")
        if saved is not None:
            env.load_state_dict(saved)
        self.model.environment = env
        return env

    def _build_bilateral(self, ckpt):
        """The BilateralGrids of a run with bilateral.enabled (default off; `--bilateral`), else None; their state restored from a
        resumed checkpoint.  Every training view gets a grid [12, L, Gh, Gw] of affine colour transforms, sliced by
        pixel position and luminance and applied to the render before the loss: what varies WITHIN a photo — vignetting, local tone
        mapping, a white balance that differs across the frame — goes into the grid and not into the Gaussians.  Inside
        [start_iteration, end_iteration) every step leaves d(loss)/dG, the total-variation term included, on the device and a
        per-view Adam updates the view's grid there; outside, the grid is applied as it is.  Held-out views have no grid and are
        scored uncorrected: `--cc-metrics` is the number to compare with a run without grids.  Composes with masks, pose
        refinement, the environment map, every background colour, both strategies and every render variant; refused beside
        exposure.enabled.  The error criterion of densification scores the uncorrected render.  The grids, moments and visit
        counts travel in the checkpoint's `native` block as tensors.  grid, lr and lambda_tv are gsplat's published settings,
        untuned here."""
        blk = self.conf["bilateral"]
        if not blk["enabled"]:
            if ckpt is not None and ckpt.get("native", {}).get("bilateral") is not None:
                # continuing without them would silently drop the transforms the Gaussians were trained against
                raise ValueError("bilateral: the checkpoint holds learnt bilateral grids and bilateral.enabled is off; resume with "
                                 "--bilateral (bilateral.enabled: true), with end_iteration 0 to keep the grids as they are")
            return None
        st = self.stepper
        require_one_gpu(st, "bilateral", "training with bilateral grids")
        if getattr(st, "enable_bilateral_gradient", None) is None or not getattr(st, "_bilateral_on", True):
            raise ValueError(f"bilateral: {type(st).__name__} leaves no grid gradient (NativeTrainStep(..., bilateral_gradient=True) does)")
        grids = bilateral_mod.BilateralGrids(len(self.train_batches), tuple(int(n) for n in blk["grid"]), self.model.raw.device,
                                             lr=float(blk["lr"]), betas=(float(blk["beta1"]), float(blk["beta2"])), eps=float(blk["eps"]),
                                             lambda_tv=float(blk["lambda_tv"]), start_iteration=int(blk["start_iteration"]),
                                             end_iteration=int(blk["end_iteration"]))
        saved = None if ckpt is None else ckpt["native"].get("bilateral")
        if saved is not None:
            grids.load_state_dict(saved)
        return grids

    def bilateral_grids(self):
        """[V,12,L,Gh,Gw] float32 host tensor: the training views' current bilateral grids, in train_batches order; None without them."""
        return None if self.bilateral is None else self.bilateral.grids()

    def environment(self):
        """[6,R,R,3] float32 host tensor: the texels of the environment map, None without one."""
        return None if self.environment_map is None else self.environment_map.texels.detach().cpu().clone()

    def exposures(self):
        """[V,3,4] float32: the training views' current colour transforms [A | b], in train_batches order (identities when exposure
        compensation is off).  Held-out views have none and are scored with the identity."""
        if self.exposure is not None:
            return self.exposure.exposures()
        return torch.tensor(exposure_mod.IDENTITY, dtype=torch.float32).reshape(1, 3, 4).repeat(len(self.train_batches), 1, 1)

    def refined_poses(self):
        """[V,4,4] float64: the training views' current camera-to-world matrices, in train_batches order (the given ones when
        pose refinement is off).  Held-out views keep their given poses and are scored there."""
        if self.refiner is not None:
            return self.refiner.refined_poses()
        return torch.stack([b.T_to_world.detach().cpu().to(torch.float64).reshape(4, 4) for b in self.train_batches])

    def _build_strategy(self, ckpt):
        from .strategy import GSStrategy, MCMCStrategy
        s, seed = self.conf["strategy"], int(self.conf["seed"])
        if self.method == "GSStrategy":
            d = s["densify"]
            gs = GSStrategy(self.stepper, clone_grad_threshold=float(d["clone_grad_threshold"]), split_grad_threshold=float(d["split_grad_threshold"]),
                            relative_size_threshold=float(d["relative_size_threshold"]), split_n_gaussians=int(d["split"]["n_gaussians"]),
                            prune_density_threshold=float(s["prune"]["density_threshold"]),
                            new_max_density=float(s["reset_density"]["new_max_density"]), density_decay_gamma=float(s["density_decay"]["gamma"]),
                            seed=seed, schedule=gs_schedule(self.conf), criterion=d["criterion"],
                            grow_fraction=float(d["error"]["grow_fraction"]), error_score=d["error"]["score"],
                            min_pixels=int(d["error"]["min_pixels"]), max_n_gaussians=d["error"]["max_n_gaussians"])
            if ckpt is not None and "densify_grad_norm_accum" in ckpt:
                dev = self.model.raw.device
                gs.grad_norm_accum = ckpt["densify_grad_norm_accum"][0].to(dev).contiguous()
                gs.grad_norm_denom = ckpt["densify_grad_norm_denom"][0].to(dev).contiguous()
            step = int(ckpt["global_step"]) if ckpt is not None else 0
            if step < gs.schedule["densify"][1]:
                gs.attach()
            return gs
        if self.method == "MCMCStrategy":
            return MCMCStrategy(self.stepper, opacity_threshold=float(s["opacity_threshold"]), binom_n_max=int(s["binom_n_max"]),
                                max_n_gaussians=int(s["add"]["max_n_gaussians"]), noise_lr=float(s["perturb"]["noise_lr"]), seed=seed,
                                schedule=mcmc_schedule(self.conf))
        raise ValueError(f"unknown strategy.method {self.method!r}")

    # ---- the loop ----
    def batch_index(self, step):
        """Index into train_batches of global step `step`: epoch step // V walks epoch_permutation(seed, epoch)."""
        n = len(self.train_batches)
        epoch = step // n
        if getattr(self, "_perm_epoch", None) != epoch:
            self._perm, self._perm_epoch = epoch_permutation(self.conf["seed"], epoch, n), epoch
        return self._perm[step % n]

    @property
    def epoch(self):
        return self.global_step // len(self.train_batches)

    def _out_dir(self):
        d = self.conf.get("out_dir") or ""
        return d or None

    def _renders_dir(self, name):
        """The directory `name` (renders_*) under the output directory, created."""
        path = os.path.join(self._out_dir(), name)
        os.makedirs(path, exist_ok=True)
        return path

    @staticmethod
    def _stem(batch, i):
        """The name of held-out view i's output files: its image's stem where main() attached one."""
        return getattr(batch, "image_stem", None) or f"{i:05d}"

    def _posed(self, view):
        """Training batch `view` at its refined pose (its pending increment applied first); the given pose without a refiner."""
        batch = self.train_batches[view]
        return batch if self.refiner is None else self.refiner.begin(view, batch)

    def _posed_batches(self, views=None):
        """The training batches (all, or those of the indices `views`) at their refined poses."""
        return [self._posed(v) for v in (range(len(self.train_batches)) if views is None else views)]

    def _sync(self):
        raw = getattr(self.model, "raw", None)
        if raw is not None and raw.is_cuda:
            torch.cuda.synchronize(raw.device)

    def _evaluation_options(self, validation=False):
        """The evaluator's keyword arguments: none with evaluation.colour_corrected and pose_alignment.enabled off (an injected
        evaluator is then called with the five positional arguments alone).  pose_aligned: the aligner's settings with the translation
        rate in world units and the run's loss weights; on validation passes only with pose_alignment.validation.

        `evaluation.colour_corrected` (default off; `--cc-metrics`) additionally scores every held-out view COLOUR-CORRECTED
        (DESIGN.md §11): the render is first mapped through the affine colour transform that fits it best to the photo, fitted on
        the device, so that a held-out photo's own exposure is not charged to the model — the number to compare an `--exposure` run
        with a run without it.  `pose_alignment.enabled` (default off; `--aligned-metrics`) additionally scores it POSE-ALIGNED
        (pose_align.PoseAligner): after a view has been scored at its given pose, that pose is optimised against the
        photo with the model frozen and the render at the best pose found is scored next to the plain one — the number to compare a
        `--refine-poses` run with a run without it.  Both leave the plain metrics as they are, need nothing from the checkpoint
        and compose with every other option; the aligner's rates and iteration count are untuned on real captures."""
        ev = self.conf["evaluation"]
        opts = dict(colour_corrected=True, ridge=float(ev["ridge"])) if ev["colour_corrected"] else {}
        pa = self.conf["pose_alignment"]
        if pa["enabled"] and (not validation or pa["validation"]):
            w = losses.loss_weights(self.conf["loss"])
            opts["pose_aligned"] = dict(iterations=int(pa["iterations"]), lr_translation=float(pa["lr_translation"]) * float(self.scene_extent),
                                        lr_rotation=float(pa["lr_rotation"]), beta1=float(pa["beta1"]), beta2=float(pa["beta2"]),
                                        eps=float(pa["eps"]), lambda_l1=w["lambda_l1"], lambda_ssim=w["lambda_ssim"])
        return opts

    def validate(self):
        """Validation pass on val_batches (trainer.py:805-842): held-out metrics and the last training loss."""
        if not self.val_batches:
            return None
        res = self.evaluator(self.model, self.tracer, self.val_batches, None, self.global_step, **self._evaluation_options(validation=True))
        loss = getattr(self, "_last_loss", None)
        entry = dict(step=self.global_step, loss=None if loss is None else float(loss), mean_psnr=res["mean_psnr"],
                     mean_ssim=res["mean_ssim"], n_gaussians=int(self.model.num_gaussians))
        entry.update({k: res[k] for k in ("mean_cc_psnr", "mean_cc_ssim") + PA_SUMMARY_KEYS if k in res})
        self.validations.append(entry)
        if self.conf.get("verbose", False):
            print(f"[trainer] step {entry['step']}: loss {entry['loss']} val psnr {entry['mean_psnr']:.3f} ssim {entry['mean_ssim']:.4f} "
                  f"N {entry['n_gaussians']}", flush=True)
        return res

    def _post_optimizer_step(self, step):
        if self.method == "MCMCStrategy":
            return self.strategy.post_optimizer_step(step, float(self.stepper.lr12[0]))
        return self.strategy.post_optimizer_step(step, self.scene_extent)

    def _error_views(self, step):
        """The training views densify step `step` scores: all of them with strategy.densify.error.views 0, otherwise that many from
        epoch_permutation(seed, step // frequency, V) — a function of the step alone, so a resumed run scores the same ones."""
        d = self.conf["strategy"]["densify"]
        n, k = len(self.train_batches), int(d["error"]["views"])
        if k == 0 or k >= n:
            return list(range(n))
        index = int(step) // max(1, int(d["frequency"]))     # (densify steps are multiples of the frequency)
        return epoch_permutation(self.conf["seed"], index, n)[:k]

    def _score_error(self, step):
        """The strategy's error_scorer (criterion "error"): the contribution scores of the live model over _error_views(step), every
        view weighted by its rendering error — at its refined pose, through its exposure row, with its mask, over the run's constant
        background (`random` is scored over black, as the held-out views are).  Nothing is kept: the next pass starts from zero.

        `strategy.densify.criterion: error` (default `gradient`; `--densify-by error`): at every densify step each
        Gaussian is charged the per-pixel error it drew (ContributionScores.accumulate_error) and the best `grow_fraction` of the
        rows by `score` are cloned or split by the reference's size rule, under `max_n_gaussians`.  The per-step gradient statistics
        are not collected, and the checkpoint holds nothing of the scores.  GSStrategy, one GPU, the unsorted variant at kernel
        degree 2 only.  grow_fraction, views and min_pixels are untuned on real captures."""
        color = self.conf["model"]["background"]["color"]
        scorer = contribution_mod.ContributionScores(self.model, self.tracer)
        env = self.environment_map
        for view in self._error_views(step):
            batch = self._posed(view)
            if self.exposure is not None:
                batch = self.exposure.begin(view, batch)
            # (an environment map: the view's own plane of it is the background the error is measured over)
            background = env.plane(batch) if env is not None else ("black" if color == "random" else color)
            scorer.accumulate_error(batch, background, mask=getattr(batch, "mask", None),
                                    exposure=getattr(batch, "exposure", None))
        return scorer.result()

    def checkpoint(self):
        return make_checkpoint(self.stepper, self.conf, self.global_step, self.epoch, self.scene_extent,
                               self.strategy if self.method == "GSStrategy" else None, self.refiner, self.exposure, self.environment_map,
                               self.bilateral)

    def save_checkpoint(self, last=False):
        out = self._out_dir()
        if out is None:
            return None
        g = self.global_step
        path = os.path.join(out, "ckpt_last.pt") if last else os.path.join(out, f"ours_{g}", f"ckpt_{g}.pt")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.checkpoint(), path)
        return path

    def train(self):
        """run_train_pass over as many epochs as n_iterations needs.  Returns the statistics table."""
        c = self.conf
        n_iter = int(c["n_iterations"])
        val_freq = max(1, int(c["val_frequency"]))
        ckpt_steps = {int(k) for k in c["checkpoint"]["iterations"]}
        start = self.global_step
        self._sync()
        t0 = time.perf_counter()
        while self.global_step < n_iter:
            g = self.global_step
            if (g > 0 or c["validate_first"]) and g % val_freq == 0:
                self.validate()
            self._step_once(g)
            self._post_optimizer_step(g)
            self.global_step = g + 1
            if self.global_step in ckpt_steps:
                self.save_checkpoint()
        self._sync()
        elapsed = time.perf_counter() - t0
        self.stats = dict(n_steps=self.global_step, n_epochs=-(-self.global_step // len(self.train_batches)), steps_run=self.global_step - start,
                          training_time=elapsed, iteration_speed=self.global_step / elapsed if elapsed > 0 else float("inf"),
                          n_gaussians=int(self.model.num_gaussians))
        if self.densify_criterion == "error":
            self.stats.update(densify_criterion="error", densify_error_passes=int(getattr(self.strategy, "error_passes", 0)),
                              densify_rows_added=int(getattr(self.strategy, "error_rows_added", 0)))
        if self.refiner is not None:
            ch = self.refiner.pose_change()
            self.stats.update(pose_mean_translation=ch["mean_translation"], pose_mean_rotation_deg=ch["mean_rotation_deg"])
        if self.exposure is not None:
            sm = self.exposure.summary()
            self.stats.update(exposure_mean_gain=sm["mean_gain"], exposure_mean_offset=sm["mean_offset"])
        if self.environment_map is not None:
            self.stats.update(environment_resolution=int(self.environment_map.resolution),
                              environment_mean_colour=self.environment_map.mean_colour())
            if self._out_dir() is not None:
                os.makedirs(self._out_dir(), exist_ok=True)
                np.save(os.path.join(self._out_dir(), "environment.npy"), self.environment().numpy())
        if self.bilateral is not None:
            sm = self.bilateral.summary()
            self.stats.update(bilateral_grid=sm["grid"], bilateral_mean_tv=sm["mean_tv"], bilateral_mean_gain=sm["mean_gain"])
            if self._out_dir() is not None:
                os.makedirs(self._out_dir(), exist_ok=True)
                np.save(os.path.join(self._out_dir(), "bilateral_grids.npy"), self.bilateral_grids().numpy())
        return self.stats

    def _step_once(self, g):
        """Global step g on its view (batch_index): the training step and the two per-view Adams behind it.  Returns the view.  The
        strategy, the step counter and the checkpoints are the caller's."""
        view = self.batch_index(g)
        self._last_loss, _ = self.stepper.step(self._train_batch(view, g))   # scheduler + SH ramp run at the end of step()
        if self.exposure is not None and self.exposure.active(g):
            self.exposure.end(view, self.stepper.exposure_gradient)   # twelve-float Adam on the device: nothing waits
        if self.refiner is not None and self.refiner.active(g):
            self.refiner.end(view, self.stepper.pose_gradient)        # queued on the device: no host synchronisation (V >= 2)
        if self.bilateral is not None and self.bilateral.active(g):
            self.bilateral.end(view, self.stepper.bilateral_gradient)   # the view's grid, one launch on the device: nothing waits
        return view

    def _train_batch(self, view, g):
        """Training batch `view` as step g trains on it: the view's refined pose and exposure row, the gradients' switches set."""
        batch = self._posed(view)
        refiner = self.refiner
        if refiner is not None:
            switch = getattr(self.stepper, "enable_pose_gradient", None)
            if switch is not None:                      # outside [start_iteration, end_iteration) the backward reduces nothing
                switch(refiner.active(g))
        comp = self.exposure
        if comp is not None:
            batch = comp.begin(view, batch)             # batch.exposure: the view's row of the device state
            switch = getattr(self.stepper, "enable_exposure_gradient", None)
            if switch is not None:                      # outside [start_iteration, end_iteration) the loss reduces nothing
                switch(comp.active(g))
        if self.environment_map is not None:            # outside [start_iteration, end_iteration) nothing is scattered or stepped
            self.stepper.environment_active = self.environment_map.active(g)
        if self.bilateral is not None:
            batch = self.bilateral.begin(view, batch)   # batch.bilateral_grid: the view's grid of the device state
            self.stepper.enable_bilateral_gradient(self.bilateral.active(g))   # outside the window the grid is applied, not learnt
        return batch

    def _compaction_mask(self, result):
        """The rows the compaction keeps, from the accumulated scores (contribution.keep_mask with the block's settings)."""
        cp = self.conf["compaction"]
        return contribution_mod.keep_mask(result, score=cp["score"], keep_fraction=float(cp["keep_fraction"]), min_pixels=int(cp["min_pixels"]))

    def compact(self):
        """The `compaction` block (default off; `--compact-to FRACTION`; DESIGN.md §13, contribution.py), after train(): every
        training view is rendered once more, at its refined pose, and each Gaussian's contribution to them is accumulated on the
        device (ContributionScores); the best `keep_fraction` of the rows by `score` stay (rows composited in fewer than
        `min_pixels` pixels go first), the others leave with their optimiser state; `finetune_iterations` further steps follow with
        the strategy detached (no densification, the learning-rate schedule continuing).  The test split is scored once more BEFORE
        the pruning, so that both sides of the trade are printed.  Fills and returns the compaction_* statistics.  One GPU only."""
        cp = self.conf["compaction"]
        before = None
        if self.test_batches:
            before = self.evaluator(self.model, self.tracer, self.test_batches, None, self.global_step, **self._evaluation_options())
        scorer = contribution_mod.ContributionScores(self.model, self.tracer)
        for batch in self._posed_batches():
            scorer.accumulate(batch)
        n_before = int(self.model.num_gaussians)
        mask = self._compaction_mask(scorer.result())
        del scorer
        detach = getattr(self.strategy, "detach", None)
        if detach is not None:
            detach()    # no densification statistics from here on
        contribution_mod.compact(self.stepper, mask, self.strategy)
        for _ in range(int(cp["finetune_iterations"])):
            self._step_once(self.global_step)      # (no strategy, no checkpoints)
            self.global_step += 1
        self._sync()
        out = dict(compaction_n_before=n_before, compaction_n_after=int(self.model.num_gaussians), compaction_score=str(cp["score"]),
                   compaction_test_psnr_before=None if before is None else float(before["mean_psnr"]))
        self.stats.update(out, n_gaussians=int(self.model.num_gaussians), n_steps=self.global_step)
        return out

    def select_by_masks(self):
        """The `selection` block (default off; `--select-by-masks [SUFFIX]`; DESIGN.md §15, selection.py), after train() and
        compact(): the label masks `<image stem><mask_suffix>.png` of the training views that have one are lifted to the Gaussians,
        at the views' refined poses (the share of each Gaussian's drawn weight inside the masks); the rows with a share above
        `threshold` and at least `min_pixels` composited pixels are selected, and the selection is rendered into every held-out view
        and scored by IoU against that view's own label mask where it has one.  With an output directory: selection.npy (bool [N]),
        selected.ply, rest.ply and renders_selection/.  Fills and returns the selection_* statistics; the model is not changed.
        One GPU only; threshold is untuned on real captures."""
        from .attributes import AttributeRenderer
        sel = self.conf["selection"]
        labelled = [v for v in range(len(self.train_batches)) if getattr(self.train_batches[v], "label_mask", None) is not None]
        if not labelled:
            raise ValueError(f"selection: no training view has a label mask (<image stem>{sel['mask_suffix']}.png next to its image)")
        lifted = selection_mod.lift_masks(self.model, self.tracer, self._posed_batches(labelled),
                                          [self.train_batches[v].label_mask for v in labelled])
        selected = selection_mod.select(lifted, threshold=float(sel["threshold"]), min_pixels=int(sel["min_pixels"]))
        out_dir = self._out_dir()
        renders = None
        if out_dir is not None:
            from .io_ply import export_native_model
            renders = self._renders_dir("renders_selection")
            np.save(os.path.join(out_dir, "selection.npy"), selected.detach().cpu().numpy().astype(bool))
            rows_in, rows_out = selection_mod.split_rows(self.model, selected)
            export_native_model(self.model, os.path.join(out_dir, "selected.ply"), rows=rows_in)
            export_native_model(self.model, os.path.join(out_dir, "rest.ply"), rows=rows_out)
        renderer = AttributeRenderer(self.model, self.tracer) if self.test_batches else None
        ious = []
        for i, batch in enumerate(self.test_batches):
            s = selection_mod.render_selection(renderer, batch, selected)
            label = getattr(batch, "label_mask", None)
            if label is not None:
                ious.append(selection_mod.mask_iou(s > 0.5, torch.as_tensor(label).reshape(s.shape) > 0.5))
            if renders is not None:
                from PIL import Image
                grey = torch.round(255.0 * s.clamp(0.0, 1.0)).to(torch.uint8).cpu().numpy()
                Image.fromarray(grey, mode="L").save(os.path.join(renders, f"{i:05d}.png"))
        out = dict(selection_n_selected=int(selected.sum()), selection_n_views_lifted=len(labelled),
                   selection_mean_iou=float(np.mean(ious)) if ious else None, selection_threshold=float(sel["threshold"]))
        self.stats.update(out)
        return out

    def fit_features(self):
        """The `features` block (default off; `--fit-features [SUFFIX]`; DESIGN.md §17, features.py), after train(), compact() and
        select_by_masks(): the maps `<image stem><suffix>.npy` (float [K,H,W] or [H,W], at the view's training resolution;
        batch.feature_map) of the training views that have one are fitted with the model frozen, at the views' refined poses, by
        `iterations` Adam steps at rate `lr`, round-robin over those views, and every held-out view that has a map is scored by the
        same mean squared error.  With an output directory: features.npy (float32 [N,K]) and renders_features/<stem>.npy (the
        held-out views' rendered planes).  Fills and returns the features_* statistics; the model is not changed.  One GPU only;
        lr and iterations are UNTUNED on real captures."""
        from .attributes import AttributeRenderer
        blk = self.conf["features"]
        mapped = [v for v in range(len(self.train_batches)) if getattr(self.train_batches[v], "feature_map", None) is not None]
        if not mapped:
            raise ValueError(f"features: no training view has a target map (<image stem>{blk['suffix']}.npy next to its image)")
        targets = [self.train_batches[v].feature_map for v in mapped]
        channels = int(targets[0].shape[0])
        for v, t in zip(mapped, targets):
            if int(t.shape[0]) != channels:
                raise ValueError(f"features: the map of training view {v} has {int(t.shape[0])} channels, the first one {channels}")
        batches = self._posed_batches(mapped)
        renderer = AttributeRenderer(self.model, self.tracer)
        feats = features_mod.fit_features(renderer, batches, targets, channels, int(blk["iterations"]), float(blk["lr"]))
        train_mse = features_mod.score_features(renderer, batches, targets, feats)
        held = [i for i, b in enumerate(self.test_batches) if getattr(b, "feature_map", None) is not None]
        for i in held:
            if int(self.test_batches[i].feature_map.shape[0]) != channels:
                raise ValueError(f"features: the map of held-out view {i} has {int(self.test_batches[i].feature_map.shape[0])} "
                                 f"channels, the training views' {channels}")
        held_mse = features_mod.score_features(renderer, [self.test_batches[i] for i in held],
                                               [self.test_batches[i].feature_map for i in held], feats) if held else None
        out_dir = self._out_dir()
        if out_dir is not None:
            renders = self._renders_dir("renders_features")
            np.save(os.path.join(out_dir, "features.npy"), feats.cpu().numpy())
            for i, batch in enumerate(self.test_batches):
                np.save(os.path.join(renders, self._stem(batch, i) + ".npy"), renderer.render(batch, feats).cpu().numpy())
        out = dict(features_channels=channels, features_n_views_fitted=len(mapped), features_train_mse=float(train_mse.mean()),
                   features_heldout_mse=None if held_mse is None else float(held_mse.mean()))
        self.stats.update(out)
        return out

    def export_points(self):
        """The `points` block (default off; `--export-points`; DESIGN.md §18, surface.py), after train(), compact(),
        select_by_masks() and fit_features(): the median surface point (the Gaussian at which the transmittance first drops below
        `level`, 0.5) of every `stride`-th pixel of every training view, at its refined pose, coloured with the rendered pixel, one
        point per cell of edge `voxel` (0: all).  With an output directory: points.ply (x y z red green blue) and
        renders_depth/<stem>.npy, the median distance of every held-out view (float32 [H,W], 0 where there is no surface).  Fills and
        returns the points_* statistics; the model is not changed.  One GPU only; stride and voxel are UNTUNED on real captures."""
        blk = self.conf["points"]
        level = float(blk["level"])
        renderer = surface_mod.SurfaceRenderer(self.model, self.tracer)
        batches = self._posed_batches()
        xyz, rgb, _ = surface_mod.fuse_points(renderer, batches, level=level, stride=int(blk["stride"]), voxel=float(blk["voxel"]))
        out_dir = self._out_dir()
        if out_dir is not None:
            from .io_ply import write_point_cloud
            renders = self._renders_dir("renders_depth")
            write_point_cloud(os.path.join(out_dir, "points.ply"), xyz.cpu().numpy(), rgb.cpu().numpy())
            for i, batch in enumerate(self.test_batches):
                np.save(os.path.join(renders, self._stem(batch, i) + ".npy"), renderer.render(batch, mode="level", level=level)["distance"].cpu().numpy())
        out = dict(points_n=int(xyz.shape[0]), points_views=len(batches), points_level=level)
        self.stats.update(out)
        return out

    def export_mesh(self):
        """The `mesh` block (default off; `--export-mesh`; DESIGN.md §19, mesh.py), after export_points(): the level-`level`
        distance planes of the training views, at their refined poses, are fused into a TSDF volume (mesh.volume_for: `bounds` or
        the 1 % .. 99 % quantile box of the positions grown by the truncation, `voxel` or the longest edge / `resolution`,
        truncation = `truncation_voxels` voxels) and its zero level is extracted by surface nets among the voxels at least
        `min_count` views updated.  With an output directory: mesh.ply (x y z red green blue, vertex_indices).  Fills and returns
        the mesh_* statistics; the model is not changed.  One GPU only; resolution, truncation_voxels and the quantile box are
        UNTUNED on real captures."""
        blk = self.conf["mesh"]
        renderer = surface_mod.SurfaceRenderer(self.model, self.tracer)
        batches = self._posed_batches()
        with torch.no_grad():
            volume = mesh_mod.volume_for(self.model, resolution=int(blk["resolution"]), voxel=blk["voxel"], bounds=blk["bounds"],
                                         truncation_voxels=float(blk["truncation_voxels"]), device=renderer.act.device)
            mesh_mod.fuse_mesh(renderer, batches, volume, level=float(blk["level"]))
            vertices, colours, faces = volume.extract(min_count=int(blk["min_count"]))
        out_dir = self._out_dir()
        if out_dir is not None:
            from .io_ply import write_mesh
            os.makedirs(out_dir, exist_ok=True)
            write_mesh(os.path.join(out_dir, "mesh.ply"), vertices.cpu().numpy(), colours.cpu().numpy(), faces.cpu().numpy())
        out = dict(mesh_vertices=int(vertices.shape[0]), mesh_faces=int(faces.shape[0]), mesh_views=int(volume.n_views),
                   mesh_voxel=float(volume.voxel), mesh_dims=[int(d) for d in volume.dims])
        self.stats.update(out)
        return out

    def run(self):
        """train(), the enabled STAGES in their order, print the statistics table, then (test_last) save ckpt_last.pt and evaluate
        the test split."""
        stats = self.train()
        for block, method, _, _ in STAGES:
            if self.conf[block]["enabled"]:
                getattr(self, method)()      # (looked up now: an instance may carry its own)
        print("Training Statistics: " + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}), flush=True)
        if self.conf["test_last"] and self.test_batches:
            self.save_checkpoint(last=True)
            self.test_metrics = self.evaluator(self.model, self.tracer, self.test_batches, self._out_dir(), self.global_step,
                                               **self._evaluation_options())
        return dict(stats=stats, test=self.test_metrics)


# The command line, in the order of --help: (flag, add_argument's keywords, the conf key it sets, how).  how "value": the value
# where the flag is given; "switch": a flag without a value, True or False into the key; "enables": as "value", and given it also
# sets `enabled` of the key's block.  No conf key: a run-level argument, read by config_from_args and main() themselves.
_UNTUNED = " (untuned on real captures)"
FLAGS = (
    ("--path", dict(required=True, help="COLMAP scene directory (sparse/0 + images[_F])"), None, None),
    ("--out-dir", {}, "out_dir", "value"),
    ("--n-iterations", dict(type=int), "n_iterations", "value"),
    ("--strategy", dict(choices=("gs", "mcmc"), default="gs"), None, None),
    ("--downsample", dict(type=int, default=1), None, None),
    ("--test-split-interval", dict(type=int, default=8), None, None),
    ("--resume", dict(default=""), None, None),
    ("--seed", dict(type=int, default=0), None, None),
    ("--background", dict(choices=BACKGROUND_COLORS, help="model.background.color (default: the config's, black); random = a uniform "
                                                          "colour per training pixel"), "model.background.color", "value"),
    ("--refine-poses", dict(help="refine the training views' camera poses while training (pose_refinement.enabled); test views keep "
                                 "theirs"), "pose_refinement.enabled", "switch"),
    ("--pose-lr-translation", dict(type=float, help="pose_refinement.lr_translation (times the scene extent)"),
     "pose_refinement.lr_translation", "value"),
    ("--pose-lr-rotation", dict(type=float, help="pose_refinement.lr_rotation (radians)"), "pose_refinement.lr_rotation", "value"),
    ("--exposure", dict(help="learn an affine colour transform per training view (exposure.enabled); test views are scored with the "
                             "identity (--cc-metrics adds colour-corrected scores)"), "exposure.enabled", "switch"),
    ("--exposure-lr", dict(type=float, help="exposure.lr"), "exposure.lr", "value"),
    ("--cc-metrics", dict(help="also score held-out views colour-corrected: through the affine colour transform fitted per view "
                               "(evaluation.colour_corrected)"), "evaluation.colour_corrected", "switch"),
    ("--aligned-metrics", dict(help="also score held-out views pose-aligned: each test view's pose is optimised against its photo with "
                                    "the model frozen before it is scored again (pose_alignment.enabled); the plain scores stay"),
     "pose_alignment.enabled", "switch"),
    ("--align-iterations", dict(type=int, help="pose_alignment.iterations"), "pose_alignment.iterations", "value"),
    ("--compact-to", dict(type=float, metavar="FRACTION", help="after training, keep this fraction of the Gaussians: the best by their "
                          "contribution to the training views (compaction.enabled, compaction.keep_fraction)"),
     "compaction.keep_fraction", "enables"),
    ("--compact-score", dict(choices=contribution_mod.SCORES, help="compaction.score"), "compaction.score", "value"),
    ("--compact-finetune", dict(type=int, metavar="K", help="compaction.finetune_iterations"), "compaction.finetune_iterations", "value"),
    ("--select-by-masks", dict(nargs="?", const=selection_mod.DEFAULTS["mask_suffix"], metavar="SUFFIX",
                               help="after training, select the Gaussians inside the views' label masks <image stem>SUFFIX.png (default "
                                    "_object), render the selection into the held-out views and score its IoU (selection.enabled, "
                                    "selection.mask_suffix)"), "selection.mask_suffix", "enables"),
    ("--select-threshold", dict(type=float, metavar="T", help="selection.threshold"), "selection.threshold", "value"),
    ("--fit-features", dict(nargs="?", const=features_mod.DEFAULTS["suffix"], metavar="SUFFIX",
                            help="after training, fit per-Gaussian features to the views' maps <image stem>SUFFIX.npy (default _features) "
                                 "with the model frozen and score them on the held-out views' maps (features.enabled, features.suffix)"),
     "features.suffix", "enables"),
    ("--feature-iterations", dict(type=int, metavar="K", help="features.iterations" + _UNTUNED), "features.iterations", "value"),
    ("--feature-lr", dict(type=float, metavar="X", help="features.lr" + _UNTUNED), "features.lr", "value"),
    ("--export-points", dict(help="after training, export the scene as points: the median surface points of the training views, fused "
                                  "into points.ply, and the held-out views' median distance planes (points.enabled)"),
     "points.enabled", "switch"),
    ("--points-level", dict(type=float, metavar="T", help="points.level: the transmittance level, 0.5 = the median"), "points.level", "value"),
    ("--points-stride", dict(type=int, metavar="S", help="points.stride: every S-th pixel" + _UNTUNED), "points.stride", "value"),
    ("--points-voxel", dict(type=float, metavar="V", help="points.voxel: one point per cell of this edge length, 0 = all" + _UNTUNED),
     "points.voxel", "value"),
    ("--export-mesh", dict(help="after training, export the scene as a triangle mesh: the training views' median distance planes fused "
                                "into a TSDF volume, its zero level written to mesh.ply (mesh.enabled)"), "mesh.enabled", "switch"),
    ("--mesh-resolution", dict(type=int, metavar="R", help="mesh.resolution: voxels along the longest edge of the box" + _UNTUNED),
     "mesh.resolution", "value"),
    ("--mesh-voxel", dict(type=float, metavar="V", help="mesh.voxel: the voxel edge length, instead of a resolution"), "mesh.voxel", "value"),
    ("--densify-by", dict(choices=("gradient", "error"), help="strategy.densify.criterion: error = grow the rows responsible for the most "
                                                              "rendering error (default: gradient)"), "strategy.densify.criterion", "value"),
    ("--densify-grow-fraction", dict(type=float, metavar="F", help="strategy.densify.error.grow_fraction"),
     "strategy.densify.error.grow_fraction", "value"),
    ("--densify-views", dict(type=int, metavar="K", help="strategy.densify.error.views: training views scored per densify step (0: all)"),
     "strategy.densify.error.views", "value"),
)
# The environment map's flags, in FLAGS' form: main() parses FLAGS + ENVIRONMENT_FLAGS.  They are a table of their own so that
# build_parser() and config_from_args() without arguments stay what they were: the conf of a command line without these flags has
# no `environment` key (resolve_config supplies the block's defaults).
ENVIRONMENT_FLAGS = (
    ("--environment", dict(help="learn an environment map: a cube-map background behind the Gaussians, composited in training and at "
                                "evaluation (environment.enabled); needs a black background"), "environment.enabled", "switch"),
    ("--environment-resolution", dict(type=int, metavar="R", help="environment.resolution: texels along a face's edge" + _UNTUNED),
     "environment.resolution", "value"),
    ("--environment-lr", dict(type=float, metavar="X", help="environment.lr" + _UNTUNED), "environment.lr", "value"),
)


# The bilateral grids' flags, likewise a table of their own: main() parses FLAGS + ENVIRONMENT_FLAGS + BILATERAL_FLAGS.
BILATERAL_FLAGS = (
    ("--bilateral", dict(help="learn a bilateral grid of affine colour transforms per training view, sliced by pixel position and "
                              "luminance (bilateral.enabled); not with --exposure; test views have no grid and are scored uncorrected: "
                              "--cc-metrics is the number to compare with a run without grids"), "bilateral.enabled", "switch"),
    ("--bilateral-grid", dict(type=int, nargs=3, metavar=("X", "Y", "L"), help="bilateral.grid: cells along x, y and luminance" + _UNTUNED),
     "bilateral.grid", "value"),
    ("--bilateral-lr", dict(type=float, metavar="X", help="bilateral.lr" + _UNTUNED), "bilateral.lr", "value"),
    ("--bilateral-tv", dict(type=float, metavar="X", help="bilateral.lambda_tv: the weight of the grids' total variation" + _UNTUNED),
     "bilateral.lambda_tv", "value"),
)
MAIN_FLAGS = FLAGS + ENVIRONMENT_FLAGS + BILATERAL_FLAGS


def build_parser(flags=FLAGS):
    ap = argparse.ArgumentParser(prog="python -m 3dgrut_amd.trainer", description="Train a COLMAP scene and score its test split.")
    for flag, keywords, _, how in flags:
        ap.add_argument(flag, **(dict(keywords, action="store_true") if how == "switch" else {"default": None, **keywords}))
    return ap


def config_from_args(a, flags=FLAGS):
    """The plain conf dict of parsed command-line arguments (build_parser(flags).parse_args(...))."""
    conf = default_config("MCMCStrategy" if a.strategy == "mcmc" else "GSStrategy")
    conf["resume"], conf["seed"] = a.resume, a.seed
    for flag, _, key, how in flags:
        value = getattr(a, flag[2:].replace("-", "_"))
        if key is None or (how != "switch" and value is None):
            continue
        *blocks, leaf = key.split(".")
        block = conf
        for name in blocks:       # (MCMCStrategy's defaults have no strategy.densify)
            block = block.setdefault(name, {})
        block[leaf] = value
        if how == "enables":
            block["enabled"] = True
    return conf


def _attach_label_masks(scene, batches, suffix):
    """batch.label_mask [H,W] of every view of `scene`: its label mask file, None where there is none."""
    for i, b in enumerate(batches):
        label = scene.load_label_mask(i, suffix)
        b.label_mask = None if label is None else torch.as_tensor(label[0, :, :, 0], device=b.rays_ori.device)


def _attach_feature_maps(scene, batches, suffix):
    """batch.feature_map [K,H,W] of every view of `scene`: its target map at the batch's resolution, None where there is none."""
    for i, b in enumerate(batches):
        fmap = scene.load_feature_map(i, suffix, size=(int(b.rays_ori.shape[2]), int(b.rays_ori.shape[1])))
        b.feature_map = None if fmap is None else torch.as_tensor(fmap, device=b.rays_ori.device)


def _attach_image_stems(scene, batches):
    """batch.image_stem of every view of `scene`: its image's file name without the extension."""
    for i, b in enumerate(batches):
        b.image_stem = os.path.splitext(os.path.basename(scene.images[i].name))[0]


def main(argv=None):
    a = build_parser(MAIN_FLAGS).parse_args(argv)
    from .io_colmap import ColmapScene
    conf = config_from_args(a, MAIN_FLAGS)
    train = ColmapScene(a.path, "train", a.downsample, a.test_split_interval)
    test = ColmapScene(a.path, "test", a.downsample, a.test_split_interval)
    # configs/initialization/colmap.yaml: observation-point scales, the model's default density / scale factor
    init = None if a.resume else train.initial_gaussians(use_observation_points=True, default_density=conf["model"]["default_density"],
                                                         default_scale_factor=conf["model"]["default_scale_factor"], seed=a.seed)
    tb = [train.batch(i) for i in range(len(train))]
    vb = [test.batch(i) for i in range(len(test))]
    for scene, batches in ((train, tb), (test, vb)):
        if conf["selection"]["enabled"]:
            _attach_label_masks(scene, batches, conf["selection"]["mask_suffix"])
        if conf["features"]["enabled"]:
            _attach_feature_maps(scene, batches, conf["features"]["suffix"])
        if conf["features"]["enabled"] or (conf["points"]["enabled"] and scene is test):   # whose outputs are named after the views
            _attach_image_stems(scene, batches)
    trainer = Trainer(conf, init, tb, val_batches=vb, test_batches=vb, scene_extent=train.cameras_extent)
    res = trainer.run()
    test_res = res["test"]
    out = dict(stats=res["stats"])
    if test_res is not None:
        out["test"] = {k: test_res[k] for k in ("mean_psnr", "std_psnr", "mean_ssim", "n_views", "mean_inference_time", "mean_cc_psnr", "std_cc_psnr",
                                                   "mean_cc_ssim") + PA_SUMMARY_KEYS if k in test_res}
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
