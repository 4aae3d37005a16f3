"""Learning per-Gaussian features from 2-D maps with the geometry frozen.

A float32 [N,K] tensor of per-Gaussian values is fitted so that its rendering (attributes.AttributeRenderer) matches
per-view target maps [K,H,W]: feature distillation, semantic or label fields, anything trained per Gaussian against 2-D maps.  The
gradient is the signed adjoint of the attribute walk (SplatRaster.trace_attributes_bwd); the model's tensors get none.

The rendered planes are premultiplied, out(p) = sum_i w(p, i) a_i with sum_i w = alpha(p), so the default loss compares them with
the premultiplied target:

    mse = mean over pixels and channels of (out - alpha * target)^2

alpha the forward's own alpha of the view, held constant.  Per view and iteration: one forward, the walk, the loss, the adjoint walk
and an Adam step, all on the device; nothing is read back inside the loop.
"""
import torch

from .confblock import boolean, check_block, integer, nonempty_string, number


def default_loss(out, alpha, target):
    """The mean over pixels and channels of (out - alpha * target)^2; out, target [K,H,W], alpha [H,W]."""
    return ((out - alpha[None] * target) ** 2).mean()


def _alpha_of(rgba):
    return rgba.detach().reshape(rgba.shape[-3], rgba.shape[-2], 4)[..., 3]


def _checked_targets(renderer, batches, targets, channels):
    if len(batches) != len(targets) or not len(batches):
        raise ValueError(f"features: {len(batches)} views and {len(targets)} target maps; at least one of each, as many of one as of the other")
    dev, out = renderer.act.device, []
    for t in targets:
        t = torch.as_tensor(t).to(device=dev, dtype=torch.float32)
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or (channels is not None and int(t.shape[0]) != int(channels)):
            raise ValueError(f"features: a target map must be [{channels if channels is not None else 'K'}, H, W], got {tuple(t.shape)}")
        out.append(t.contiguous())
    return out


def fit_features(renderer, batches, targets, channels, iterations, lr, init=None, loss=None):
    """Fits float32 [N, channels] features of the renderer's rows to `targets` (one [K,H,W] map per batch, on any device) with
    torch.optim.Adam, visiting the views round-robin, `iterations` steps in all.  init: the starting values (zeros otherwise);
    loss: a callable on (out [K,H,W], alpha [H,W], target [K,H,W]) returning a scalar, default_loss otherwise.  Returns the fitted
    tensor, detached, on the renderer's device."""
    channels, iterations = int(channels), int(iterations)
    if not 1 <= channels <= 64:
        raise ValueError(f"features: between 1 and 64 channels, got {channels}")
    targets = _checked_targets(renderer, batches, targets, channels)
    n, dev = int(renderer.act.shape[0]), renderer.act.device
    if init is None:
        feats = torch.zeros((n, channels), dtype=torch.float32, device=dev)
    else:
        feats = torch.as_tensor(init).detach().to(device=dev, dtype=torch.float32).clone().contiguous()
        if tuple(feats.shape) != (n, channels):
            raise ValueError(f"features: init must be [{n}, {channels}], got {tuple(feats.shape)}")
    feats.requires_grad_(True)
    loss = default_loss if loss is None else loss
    opt = torch.optim.Adam([feats], lr=float(lr))
    for it in range(iterations):
        v = it % len(batches)
        rgba, out = renderer.render_with_image(batches[v], feats)
        if tuple(out.shape) != tuple(targets[v].shape):
            raise ValueError(f"features: view {v} renders {tuple(out.shape)}, its target map is {tuple(targets[v].shape)}")
        opt.zero_grad(set_to_none=True)
        loss(out, _alpha_of(rgba), targets[v]).backward()
        opt.step()
    return feats.detach()


def score_features(renderer, batches, targets, features):
    """default_loss of every view, a float64 tensor [len(batches)] on the renderer's device (nothing is read back)."""
    k = int(torch.as_tensor(features).shape[-1]) if torch.as_tensor(features).dim() == 2 else 1
    targets = _checked_targets(renderer, batches, targets, k)
    scores = []
    with torch.no_grad():
        for batch, target in zip(batches, targets):
            rgba, out = renderer.render_with_image(batch, features)
            if tuple(out.shape) != tuple(target.shape):
                raise ValueError(f"features: a view renders {tuple(out.shape)}, its target map is {tuple(target.shape)}")
            scores.append(default_loss(out.double(), _alpha_of(rgba).double(), target.double()))
    return torch.stack(scores)


# the trainer's `features` block
DEFAULTS = {"enabled": False, "suffix": "_features", "iterations": 200, "lr": 0.03}
RULES = {"enabled": boolean(), "suffix": nonempty_string(), "iterations": integer(ge=1), "lr": number("a number > 0", gt=0)}


def check_config(block):
    """The resolved `features` block: enabled true or false, suffix a non-empty string, iterations an integer >= 1, lr > 0."""
    return check_block("features", block, DEFAULTS, RULES)
