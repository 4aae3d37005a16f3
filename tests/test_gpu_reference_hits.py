"""K7 against sums of the reference's OWN per-hit gradients.

Scene (c) of tests/golden/hit_golden.npz (tests/golden/gen_hit_golden.py): one 48 x 40 view of 12 Gaussians per kernel degree, whose
[12,12] and [12,48] gradients were accumulated in float64 from what the reference's processHitBwd / radianceFromSpHBwd, compiled for
the host, returned hit by hit along the oracle's tile lists.  The activated rows go through SplatRaster.trace / trace_bwd with
render.particle_kernel_degree set (degree 2: the default compositors of gut_render.hip; the others: gut_render_general.hip) and
every row must sit inside its own bound (tests/common.check_gradients_per_row, budget from oracle.backward(flip_bound=ROW_FLIP_BOUND),
constants as they stand).  The tests read the fixture only: neither the reference tree nor the library built from it.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import reference_hit_cases as rc
from tests.common import FLIP_MARGIN_BOUND, ROW_FLIP_BOUND, cams, check_gradients_per_row, check_tile_traversal, make_view, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    with np.load(rc.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_backward_against_the_reference_per_hit_sums(golden, degree):
    W, H, sh = rc.SCENE_W, rc.SCENE_H, rc.SCENE_SH_DEGREE
    view = make_view("pinhole", W, H, cams.look_at_c2w(rc.SCENE_EYE, rc.SCENE_TARGET), fx=rc.SCENE_FX)
    d12, sph, rgba_grad, dist_grad = (golden[k] for k in ("scene_d12", "scene_sph", "scene_rgba_grad", "scene_dist_grad"))
    prm = oracle.default_params(); prm.kernel_degree = degree
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=sh, params=prm)
    _, _, _, budget = oracle.backward(view["oracle_cam"], ref, rgba_grad, dist_grad, params=prm, flip_bound=ROW_FLIP_BOUND)
    margins = oracle.render_margins(view["oracle_cam"], ref, params=prm)

    tr = gut.Tracer({"render": {"particle_kernel_degree": degree}})
    raster = tr.tracer_wrapper
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    d12_t, sph_t = torch.as_tensor(d12, device=DEV).contiguous(), torch.as_tensor(sph, device=DEV).contiguous()
    cam = (ro, rd, None, sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
    rgba, dist, hits, _ = raster.trace(0, sh, d12_t, sph_t, *cam)
    g12, g48 = raster.trace_bwd(0, sh, d12_t, sph_t, *cam, rgba, torch.as_tensor(rgba_grad, device=DEV), dist, torch.as_tensor(dist_grad, device=DEV))
    label = f"reference per-hit sums, kernel degree {degree}"
    assert np.array_equal(raster.debug_buffer("sorted_ids").cpu().numpy().view(np.uint32), ref["sorted_ids"]), "the walk is over other tile lists"
    check_gradients_per_row(g12.cpu().numpy(), g48.cpu().numpy(), golden[f"scene{degree}_g12"], golden[f"scene{degree}_g48"], label, budget, sh_degree=sh)

    # the walk itself: hit counts per pixel and traversal depths per tile wherever no decision is flip-prone; with no flip-prone pixel
    # at all, the number of accepted (ray, entry) pairs is the fixture's and the traversal total the oracle's
    hits_np = hits.cpu().numpy()
    calm = margins.min(-1) >= FLIP_MARGIN_BOUND
    assert np.array_equal(hits_np.reshape(H, W)[calm], ref["hits"].reshape(H, W)[calm]), f"{label}: hit counts differ where no decision is near a threshold"
    check_tile_traversal(raster.debug_buffer("tile_traversed_bwd").cpu().numpy().view(np.uint32), ref["tile_traversed_bwd"], margins, W, H, label)
    prone = int((~calm).sum())
    pairs = int(golden[f"scene{degree}_pairs"])
    print(f"[{label}] {prone} flip-prone pixels; accepted pairs: GPU {int(hits_np.sum())}, fixture {pairs}; traversed_bwd {raster.stats()['traversed_bwd']} / {ref['traversed_bwd']}")
    if prone == 0:
        assert int(hits_np.sum()) == pairs
        assert raster.stats()["traversed_bwd"] == ref["traversed_bwd"]
