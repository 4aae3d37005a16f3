"""The preconditions of tests/test_gpu_off_centre_rays.py, on the CPU oracle and float64 alone (tests/off_centre_cases.py: the
origin planes).  Before the device is compared with the oracle on rays that do not start at the sensor position, the oracle itself is
held to float64 there, forward and backward, and the tolerance model the GPU tests use is measured there:

  * every case x plane of the GPU file really moves the image (by more than 100 x COLOUR_TOL) and moves nothing K1 writes;
  * the oracle's forward against per_ray_torch.render_tiled, at the bar of test_c_oracle_matches_float64_autograd;
  * the oracle's backward against float64 autograd of the same restatement, rows 0..11 and the SH rows, with and without a
    distance cotangent (the reference's hit-distance backward: per_ray_torch._ReferenceHitDistance) — what pins the oracle's own
    e terms;
  * the two-evaluation band of test_two_fp32_evaluations_measure_the_tolerance_model on the three small scenes x three planes;
  * the pose identity of tests/test_cpu_pose_gradient.py for off-centre rays."""
import importlib

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import off_centre_cases as oc
from tests import test_cpu_oracle as t_oracle
from tests import test_cpu_pose_gradient as t_pose
from tests.common import COLOUR_TOL, cams, densified_like_scene, make_view, pose, scenes

oracle = importlib.import_module("oracle.oracle")
prt = importlib.import_module("oracle.per_ray_torch")

K1_KEYS = ("tiles_count", "tiles_offset", "unsorted_ids", "sorted_ids", "unsorted_keys", "sorted_keys", "tile_ranges", "proj_pos",
           "conic_opacity", "extent", "depth", "feat", "visibility")


def _parity_case(name):
    mk, kind, W, H, (eye, tgt), kw = importlib.import_module("tests.test_gpu_parity").CASES[name]
    sc = mk()
    return scenes.pack_density(sc), sc["features"], make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw), {}


def _walk_case(name):
    c = cr._base(name)
    return c["d12"], c["sph"], c["view"], {}


def _rolling_case():
    sc = scenes.scene_c1(700, 41)
    view = make_view("pinhole", 96, 80, cams.look_at_c2w((0.1, 0.0, -3.0), (0, 0, 0)), fx=90)
    tq_end = pose.sensor_pose_from_c2w(cams.look_at_c2w((0.25, -0.1, -2.9), (0.05, 0.0, 0.0))).T_world_sensors[0]
    return scenes.pack_density(sc), sc["features"], view, dict(shutter=1, pose_end=tq_end)


def _pose_case():
    sc = scenes.scene_c1(1000, 0)
    return scenes.pack_density(sc), sc["features"], make_view("pinhole", 128, 128, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0))), {}


def _scale_case():
    sc = densified_like_scene(200000, 5)
    return scenes.pack_density(sc), sc["features"], make_view("pinhole", 720, 720, cams.orbit_c2w(3.6, -40, 25), fx=945.0), {}


USED = ([(f"{name}/{plane}", (lambda name=name: _parity_case(name)), plane)
         for name in ("c1_pinhole_128", "ragged_100x70", "fisheye_distorted", "dense_big_splats") for plane in ("shift", "sweep", "half")]
        + [(f"{name}/{plane}", (lambda name=name: _walk_case(name)), plane)
           for name in ("pinhole_64x48", "ragged_70x45", "fisheye") for plane in ("shift", "sweep")]
        + [("rolling_shutter/shift", _rolling_case, "shift"), ("pose_128/shift", _pose_case, "shift"),
           ("densified_200k_720/shift", _scale_case, "shift"), ("densified_200k_720/sweep", _scale_case, "sweep")])


@pytest.mark.parametrize("label,make,plane", USED, ids=[u[0] for u in USED])
def test_every_used_plane_moves_the_image_and_nothing_of_the_binning(label, make, plane):
    d12, sph, view0, cam_edit = make()
    view = oc.off_centre(view0, plane)
    assert view["ro"].shape == view0["ro"].shape and view["ro"].dtype == view0["ro"].dtype == np.float32
    assert view["rd"] is view0["rd"] and not view0["ro"].any()
    W, H = view["W"], view["H"]
    a = oracle.forward(dict(view0["oracle_cam"], **cam_edit), W, H, d12, sph, view0["ro"], view0["rd"], sh_degree=3)
    b = oracle.forward(dict(view["oracle_cam"], **cam_edit), W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    moved = float(np.abs(a["rgba"] - b["rgba"]).max())
    print(f"[off-centre {label}] the oracle's image moves by {moved:.3f}; {int(oc.uncentred_tiles(view).sum())} of {oc.uncentred_tiles(view).size} tiles un-centred")
    assert moved > 100 * COLOUR_TOL
    assert a["M"] == b["M"] > 0
    for key in K1_KEYS:       # K1 reads no rays
        assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint8), np.ascontiguousarray(b[key]).view(np.uint8)), key


def test_the_planes_are_what_the_table_says():
    view = make_view("pinhole", 128, 128, cams.look_at_c2w((0, 0, -4), (0, 0, 0)), fx=128)
    shift, sweep, half, nz = (oc.off_centre(view, p) for p in oc.PLANES)
    assert oc.uncentred_tiles(shift).all() and np.array_equal(np.unique(shift["ro"].reshape(-1, 3), axis=0), np.asarray([oc.SHIFT], np.float32))
    un = oc.uncentred_tiles(sweep)
    rows = sweep["ro"].reshape(128, 128, 3)
    assert un.all() and int((rows == 0).all(-1).sum()) == 1 and not rows[64, 64].any()    # one ray starts at the sensor: its tile is mixed
    assert len(np.unique(rows[:, 0, 0])) == 128 and len(np.unique(rows[0, :, 1])) == 128 and not rows[..., 2].any()
    un = oc.uncentred_tiles(half)
    assert not un[:, :2].any() and un[:, 2:].all()
    h = half["ro"].reshape(128, 128, 3)
    assert not h[:, :oc.HALF_CUT].any() and (h[:, oc.HALF_CUT:] == np.asarray(oc.SHIFT, np.float32)).all()
    assert 32 < oc.HALF_CUT < 48                                                 # the cut runs through the tile column 32..47
    assert np.signbit(nz["ro"]).all() and not nz["ro"].any() and not oc.uncentred_tiles(nz).any()
    # a ragged image: tiles cut by the right and bottom edge
    r = oc.off_centre(make_view("pinhole", 100, 70, cams.look_at_c2w((0, 0, -4), (0, 0, 0)), fx=90), "half")
    assert oc.uncentred_tiles(r).shape == (5, 7) and not oc.uncentred_tiles(r)[:, :2].any() and oc.uncentred_tiles(r)[:, 2:].all()


@pytest.mark.parametrize("plane", ["shift", "sweep", "half"])
@pytest.mark.parametrize("kind", ["pinhole", "fisheye"])
def test_oracle_forward_matches_float64_off_centre(kind, plane):
    """test_c_oracle_matches_float64_autograd's scene, views and bars: colours to 2e-5, hit counts equal."""
    sc = scenes.scene_c1(250, seed=5)
    W, H = 48, 40
    view = make_view(kind, W, H, cams.look_at_c2w((0.3, 0.2, -3.5 if kind == "pinhole" else -2.0), (0, 0, 0)), fx=50 if kind == "pinhole" else None)
    view = oc.off_centre(view, plane)
    f = oracle.forward(view["oracle_cam"], W, H, scenes.pack_density(sc), sc["features"], view["ro"], view["rd"])
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in sc.items()}
    rgba, dist, hits = prt.render_tiled(params, view["tq"], W, H, view["ro"], view["rd"], f["tile_ranges"], f["sorted_ids"])
    err = float(np.abs(rgba.numpy() - f["rgba"]).max())
    print(f"[oracle forward off-centre {kind}/{plane}] {err:.2e} from float64")
    assert err <= 2e-5
    assert np.abs(hits.numpy() - f["hits"][..., 0]).max() == 0


@pytest.mark.parametrize("with_dist", [False, True])
@pytest.mark.parametrize("plane", ["shift", "sweep"])
def test_oracle_backward_matches_float64_autograd_off_centre(plane, with_dist):
    """scene_c1(300, 0) at 64 x 48 (the case of the pose identity and of the walks).  Every block to 5e-5 of its largest entry, the bar
    of test_c_oracle_matches_float64_autograd; with a distance cotangent the float64 side differentiates the hit distance as the
    reference does (diagonal terms only), everything else as autograd does."""
    sc = scenes.scene_c1(300, 0)
    W, H = 64, 48
    view = oc.off_centre(make_view("pinhole", W, H, cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0)), fx=64.0), plane)
    f = oracle.forward(view["oracle_cam"], W, H, scenes.pack_density(sc), sc["features"], view["ro"], view["rd"])
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sc.items()}
    rgba, dist, hits = prt.render_tiled(params, view["tq"], W, H, view["ro"], view["rd"], f["tile_ranges"], f["sorted_ids"],
                                        reference_hit_distance_grad=with_dist)
    assert np.abs(rgba.detach().numpy() - f["rgba"]).max() <= 2e-5 and np.abs(hits.numpy() - f["hits"][..., 0]).max() == 0
    rng = np.random.default_rng(0)
    rg = rng.normal(size=(H, W, 4)).astype(np.float32)
    dg = (0.1 * rng.normal(size=(H, W, 1))).astype(np.float32) if with_dist else np.zeros((H, W, 1), np.float32)
    loss = (rgba * torch.tensor(rg, dtype=torch.float64)).sum()
    if with_dist:
        loss = loss + (dist * torch.tensor(dg[..., 0], dtype=torch.float64)).sum()
    loss.backward()
    g12, g48, _ = oracle.backward(view["oracle_cam"], f, rg, dg)
    rel = lambda a, b: float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
    errs = dict(positions=rel(params["positions"].grad.numpy(), g12[:, 0:3]), density=rel(params["density"].grad.numpy()[:, 0], g12[:, 3]),
                rotation=rel(params["rotation"].grad.numpy(), g12[:, 4:8]), scale=rel(params["scale"].grad.numpy(), g12[:, 8:11]),
                sh=rel(params["features"].grad.numpy(), g48))
    print(f"[oracle backward off-centre {plane}/dist={int(with_dist)}] {errs}")
    assert not g12[:, 11].any()
    for block, err in errs.items():
        assert err <= 5e-5, (block, err)
    if with_dist:     # the distance cotangent reaches the rows: without it they differ
        g12_0, _, _ = oracle.backward(view["oracle_cam"], f, rg, np.zeros((H, W, 1), np.float32))
        assert rel(g12_0[:, 8:11], g12[:, 8:11]) > 1e-3


@pytest.mark.parametrize("plane", ["shift", "sweep", "half"])
@pytest.mark.parametrize("name", ["c1_pinhole_128", "fisheye_distorted", "dense_big_splats"])
def test_tolerance_model_holds_off_centre(name, plane):
    """test_two_fp32_evaluations_measure_the_tolerance_model's body (every constant divided by K_BAND, every pixel, every row) with
    the view's origin plane replaced."""
    mk, kind, W, H, c2w, kw = t_oracle.BAND_SCENES[name]
    t_oracle.check_tolerance_band(f"{name}/{plane}", mk(), oc.off_centre(make_view(kind, W, H, c2w(), **kw), plane))


@pytest.mark.parametrize("sh_degree", [3, 0])
def test_pose_identity_for_off_centre_rays(sh_degree):
    """The twist case with the `shift` plane: a rigid twist about the camera centre moves the rays' origins too (o_c' = R rho + A o_c),
    and the reduction of the Gaussian gradients about the camera centre still equals autograd to 1e-7."""
    auto, act, grad, cam_pos = t_pose._twist_case(sh_degree, plane="shift")
    centred = t_pose._twist_case(sh_degree)[0]
    got = -pose.pose_gradient_from_rows(act, grad, cam_pos)
    scale = float(auto.abs().max())
    err = float((got - auto).abs().max()) / scale
    print(f"[pose identity off-centre, SH degree {sh_degree}] autograd {auto.tolist()} error {err:.3e} of the largest component")
    assert scale > 0 and err <= 1e-7, err
    assert float((auto - centred).abs().max()) > 1e-3 * scale       # another loss than the centred case's
