"""The CPU reference of the attribute walk (gut_trace_attributes) on the cases of tests/contribution_reference.py, and
the selection pipeline of 3dgrut_amd/selection.py on the reference alone.

`attribute_reference(cam, fwd, attrs, params)` is the loop of weighted_contribution_reference.weighted_reference transposed: per
pixel, oracle.debug_ray gives the accepted entries and their weights w, and out[:, py, px] = sum of w * attrs[id].
`attribute_case(name)` adds, per case, seeded attributes in [0, 1] (K = 4, the last channel all ones), their reference planes and
the case's per-pixel flip budget.  `selection_case()` is the selection pipeline — lift from two views, select, render into a third —
in float64 from these references, with what the device test needs to say where the device may differ.

Everything is computed once and cached: the tests share it and leave it unchanged."""
import functools
import importlib

import numpy as np

from tests import contribution_reference as cr
from tests import weighted_contribution_reference as wr
from tests.common import COLOUR_TOL, PIX_FLIP, ROW_FLIP_BOUND, cams, make_view, scenes

oracle = importlib.import_module("oracle.oracle")
selection = importlib.import_module("3dgrut_amd.selection")


def attribute_reference(cam, fwd, attrs, params=None):
    """out [K,H,W] float64 with out[:, py, px] = the sum over the pixel's accepted entries of w * attrs[id]; attrs [N,K]."""
    d12, _, _, _, _, W, H = fwd["_inputs"]
    a = np.asarray(attrs, np.float64)
    assert a.ndim == 2 and a.shape[0] == d12.shape[0]
    out = np.zeros((a.shape[1], H, W))
    longest = int((fwd["tile_ranges"][:, 1].astype(np.int64) - fwd["tile_ranges"][:, 0]).max()) if fwd["M"] else 0
    for py in range(H if fwd["M"] else 0):
        for px in range(W):
            e = oracle.debug_ray(cam, fwd, px, py, params=params, max_entries=max(16, longest))
            if not len(e):
                continue
            acc = e[:, 5] != 0
            if not acc.any():
                continue
            t_after = e[acc, 6]
            w = np.concatenate([[1.0], t_after[:-1]]) * e[acc, 3]
            out[:, py, px] = w @ a[e[acc, 0].astype(np.int64)]
    return out


def random_attributes(name, n, k=4):
    """Seeded uniform [0, 1) attributes float32 [n, k], the last channel all ones."""
    a = np.random.default_rng(70 + cr.case_index(name)).uniform(0, 1, (n, k)).astype(np.float32)
    a[:, -1] = 1.0
    return a


@functools.lru_cache(maxsize=None)
def attribute_case(name):
    """dict(attrs float32 [N,4], planes float64 [4,H,W], margins [H,W,2], budget [H,W,2]) of the named case."""
    c = cr.case(name)
    cam, fwd = c["view"]["oracle_cam"], c["ref"]
    prm = c["params"]()
    attrs = random_attributes(name, c["d12"].shape[0])
    planes = attribute_reference(cam, fwd, attrs, params=prm)
    margins, budget = oracle.render_margins(cam, fwd, params=prm, budget_bound=ROW_FLIP_BOUND)
    return dict(attrs=attrs, planes=planes, margins=margins, budget=budget)


# ---- the selection pipeline on the reference ----
SELECTION_VIEWS = (("lift", cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0))),
                   ("lift", cams.orbit_c2w(4.0, 37.0, 12.0)),
                   ("held_out", cams.orbit_c2w(4.0, -25.0, 5.0)))
SELECTION_SIZE = (64, 48)


@functools.lru_cache(maxsize=None)
def selection_case():
    """scene_c1(300, 0), three pinhole views at 64 x 48 (two to lift from, one held out), truth = position.x < 0, label masks =
    attribute_reference(truth) > 0.5.  dict(scene, d12, sph, views, truth, labels [3][H,W] bool, lifted (share, weight_sum, pixels,
    n_views as numpy), row_slack [N] (how far from the threshold a row's share must lie for the device to be held to the reference's
    decision), selected [N] bool, s [H,W] float64 of the held-out view, pixel_slack [H,W], pred, iou, agreement)."""
    W, H = SELECTION_SIZE
    sc = scenes.scene_c1(300, 0)
    d12 = np.ascontiguousarray(scenes.pack_density(sc))
    sph = np.ascontiguousarray(sc["features"].astype(np.float32))
    n = d12.shape[0]
    truth = np.asarray(sc["positions"])[:, 0] < 0
    views = [make_view("pinhole", W, H, c2w, fx=1.0 * W) for _, c2w in SELECTION_VIEWS]
    fwds = [oracle.forward(v["oracle_cam"], W, H, d12, sph, v["ro"], v["rd"], sh_degree=3) for v in views]
    labels = [attribute_reference(v["oracle_cam"], f, truth[:, None].astype(np.float64))[0] > 0.5 for v, f in zip(views, fwds)]
    weighted, weight, pixels, row_budget = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    for v, f, lab in zip(views[:2], fwds[:2], labels[:2]):
        sums = wr.weighted_reference(v["oracle_cam"], f, np.stack([np.ones((H, W)), lab.astype(np.float64)]))
        weight += sums[0]
        weighted += sums[1]
        pixels += cr.reference(v["oracle_cam"], f)["pixels"]
        cot = np.zeros((H, W, 4), np.float32)
        cot[..., 0] = 1.0           # the flip budget of the plain sum bounds the weighted one's: every factor is at most 1
        _, _, _, budget = oracle.backward(v["oracle_cam"], f, cot, np.zeros((H, W, 1), np.float32), flip_bound=ROW_FLIP_BOUND)
        row_budget += budget[:, 4]
    lifted = dict(share=selection.share_of(weighted, weight), weight_sum=weight, pixels=pixels, n_views=2)
    selected = selection.select(lifted, threshold=0.5, min_pixels=1)
    row_slack = (PIX_FLIP * row_budget + COLOUR_TOL * pixels) / np.where(weight > 0, weight, 1.0)
    s = attribute_reference(views[2]["oracle_cam"], fwds[2], selected[:, None].astype(np.float64))[0]
    _, pix_budget = oracle.render_margins(views[2]["oracle_cam"], fwds[2], budget_bound=ROW_FLIP_BOUND)
    pixel_slack = COLOUR_TOL + PIX_FLIP * pix_budget[..., 0].astype(np.float64)
    pred = s > 0.5
    scored = pixels >= 1
    return dict(scene=sc, d12=d12, sph=sph, views=views, fwds=fwds, truth=truth, labels=labels, lifted=lifted, row_slack=row_slack,
                selected=selected, s=s, pixel_slack=pixel_slack, pred=pred, iou=selection.mask_iou(pred, labels[2]),
                agreement=float((selected[scored] == truth[scored]).mean()), scored=scored)
