"""Rendering per-Gaussian attributes into views.

Any quantity stored per Gaussian — a label, a score, a selection, a feature vector — is blended into a view with the weights
w = T * alpha the forward compositor forms for the view's colours:

    out[k, pixel] = sum over the Gaussians composited in the pixel of w * attributes[i, k]

by SplatRaster.trace_attributes (gut_trace_attributes): the forward's walk once more, four channels per walk.  It is the other
direction of the weighted contribution walk (contribution.ContributionScores.accumulate with a plane), which sums a
per-pixel plane onto the Gaussians with the same weights: for a plane P in [0, 1],  sum_p P(p) out(p) = sum_i a_i weighted_sum_i(P).
A channel of ones renders the view's alpha; a 0/1 selection renders, per pixel, how much of it the selected Gaussians draw.

`AttributeRenderer` holds the model's rows activated and packed once (contribution.FrozenModel, as ContributionScores does) and
renders per view with one forward and the walk, nothing read back.  Nothing here is differentiable.
"""
import torch

from .contribution import FrozenModel


class AttributeRenderer(FrozenModel):
    """Renders attributes of `model`'s rows into the views handed to render(); the model must not change meanwhile."""

    def as_rows(self, attributes):
        """attributes as the contiguous float32 [N,K] tensor on the model's device the walk reads: a 1-D [N] tensor is one channel;
        bool and integer tensors (and other float types) are converted."""
        a = torch.as_tensor(attributes)
        if a.dim() == 1:
            a = a[:, None]
        n = int(self.act.shape[0])
        if a.dim() != 2 or a.shape[0] != n:
            raise ValueError(f"attributes must be [{n}] or [{n}, K], got {tuple(a.shape)}")
        if not 1 <= int(a.shape[1]) <= 64:
            raise ValueError(f"attributes: between 1 and 64 channels, got {int(a.shape[1])}")
        return a.detach().to(device=self.act.device, dtype=torch.float32).contiguous()

    def render_with_image(self, batch, attributes, out=None):
        """(rgba [1,H,W,4] of the forward, the attribute planes float32 [K,H,W]) of the batch's view."""
        rows = self.as_rows(attributes)
        outs, rays_o, rays_d, cam = self.forward(batch)
        planes = self.raster.trace_attributes(0, self.n_active_features, self.act, rows, rays_o, rays_d, *cam, out=out)
        return outs[0], planes

    def render(self, batch, attributes, out=None):
        """The attribute planes float32 [K,H,W] of the batch's view: one forward plus the walk, nothing read back."""
        return self.render_with_image(batch, attributes, out=out)[1]
