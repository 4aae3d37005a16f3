"""Rendering per-Gaussian attributes into views.

Any quantity stored per Gaussian — a label, a score, a selection, a feature vector — is blended into a view with the weights
w = T * alpha the forward compositor forms for the view's colours:

    out[k, pixel] = sum over the Gaussians composited in the pixel of w * attributes[i, k]

by SplatRaster.trace_attributes (gut_trace_attributes): the forward's walk once more, four channels per walk.  It is the other
direction of the weighted contribution walk (contribution.ContributionScores.accumulate with a plane), which sums a
per-pixel plane onto the Gaussians with the same weights: for a plane P in [0, 1],  sum_p P(p) out(p) = sum_i a_i weighted_sum_i(P).
A channel of ones renders the view's alpha; a 0/1 selection renders, per pixel, how much of it the selected Gaussians draw.

`AttributeRenderer` holds the model's rows activated and packed once (contribution.FrozenModel, as ContributionScores does) and
renders per view with one forward and the walk, nothing read back.  Since DESIGN.md §17 the planes are differentiable with respect
to the ATTRIBUTES (SplatRaster.trace_attributes_bwd, the signed adjoint of the walk); the geometry is frozen and gets no gradient.
"""
import torch

from .contribution import FrozenModel


class _RenderAttributes(torch.autograd.Function):
    """rows [N,K] -> (planes [K,H,W], rgba of the forward).  The backward is SplatRaster.trace_attributes_bwd on the cotangent of the
    planes and returns the gradient of the rows ONLY: the renderer's model is frozen (its rows were activated and packed once,
    outside any graph), so no model tensor receives a gradient through the planes, and rgba is not differentiable here.  The walk
    follows the handle's cached forward: if the renderer has rendered anything since this node's forward, the backward first runs
    the forward of its own batch again (the rows are frozen, so it rebuilds the very lists the planes were rendered from)."""

    @staticmethod
    def forward(ctx, rows, renderer, batch, out):
        outs, rays_o, rays_d, cam = renderer.forward(batch)
        planes = renderer.raster.trace_attributes(0, renderer.n_active_features, renderer.act, rows, rays_o, rays_d, *cam, out=out)
        ctx.renderer, ctx.batch, ctx.call, ctx.stamp = renderer, batch, (rays_o, rays_d, cam), renderer.n_forwards
        ctx.mark_non_differentiable(outs[0])
        return planes, outs[0]

    @staticmethod
    def backward(ctx, planes_grad, _rgba_grad):
        renderer = ctx.renderer
        rays_o, rays_d, cam = ctx.call
        if renderer.n_forwards != ctx.stamp:
            _, rays_o, rays_d, cam = renderer.forward(ctx.batch)
        g = planes_grad.to(torch.float32).contiguous()
        grad = renderer.raster.trace_attributes_bwd(0, renderer.n_active_features, renderer.act, g, rays_o, rays_d, *cam)
        return grad, None, None, None


class AttributeRenderer(FrozenModel):
    """Renders attributes of `model`'s rows into the views handed to render(); the model must not change meanwhile."""

    def _shaped(self, attributes):
        a = torch.as_tensor(attributes)
        if a.dim() == 1:
            a = a[:, None]
        n = int(self.act.shape[0])
        if a.dim() != 2 or a.shape[0] != n:
            raise ValueError(f"attributes must be [{n}] or [{n}, K], got {tuple(a.shape)}")
        if not 1 <= int(a.shape[1]) <= 64:
            raise ValueError(f"attributes: between 1 and 64 channels, got {int(a.shape[1])}")
        return a

    def as_rows(self, attributes):
        """attributes as the contiguous float32 [N,K] tensor on the model's device the walk reads: a 1-D [N] tensor is one channel;
        bool and integer tensors (and other float types) are converted."""
        return self._shaped(attributes).detach().to(device=self.act.device, dtype=torch.float32).contiguous()

    def render_with_image(self, batch, attributes, out=None):
        """(rgba [1,H,W,4] of the forward, the attribute planes float32 [K,H,W]) of the batch's view.  Where `attributes` requires a
        gradient (and gradients are enabled) the planes carry a graph whose backward gives the gradient of the attributes alone —
        the model's tensors get none, the geometry is frozen; otherwise nothing is recorded."""
        if isinstance(attributes, torch.Tensor) and attributes.requires_grad and torch.is_grad_enabled():
            rows = self._shaped(attributes).to(device=self.act.device, dtype=torch.float32).contiguous()
            planes, rgba = _RenderAttributes.apply(rows, self, batch, out)
            return rgba, planes
        rows = self.as_rows(attributes)
        outs, rays_o, rays_d, cam = self.forward(batch)
        planes = self.raster.trace_attributes(0, self.n_active_features, self.act, rows, rays_o, rays_d, *cam, out=out)
        return outs[0], planes

    def render(self, batch, attributes, out=None):
        """The attribute planes float32 [K,H,W] of the batch's view: one forward plus the walk, nothing read back."""
        return self.render_with_image(batch, attributes, out=out)[1]
