"""The mesh export on the device: gut_tsdf_integrate against the float64 reference voxel by voxel, its exact
properties (order, batching, repetition), the surface nets against the reference on the same integer grid, the sphere end to end,
the wall through the renderer, the refusals, the trainer's command line."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_reference as mr
from tests import surface_reference as sr
from tests.common import COLOUR_TOL, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
io_ply = importlib.import_module("3dgrut_amd.io_ply")
mesh = importlib.import_module("3dgrut_amd.mesh")
native = importlib.import_module("3dgrut_amd.native")
surface = importlib.import_module("3dgrut_amd.surface")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
_capi = importlib.import_module("3dgrut_amd._capi")
DEV = "cuda:0"
STATE = ("acc", "cnt", "rgb_sum", "rgb_cnt")


def _camera(view, moving=False):
    cam = _capi.GutCamera()
    cam.model = _capi.CAMERA_FISHEYE if view["model"] == "fisheye" else _capi.CAMERA_PINHOLE
    cam.shutter = _capi.SHUTTER_GLOBAL
    cam.principal_point[:] = [float(v) for v in view["principal_point"]]
    cam.focal_length[:] = [float(v) for v in view["focal_length"]]
    cam.radial_coeffs[:] = [float(v) for v in view["radial"]]
    cam.tangential_coeffs[:] = [float(v) for v in view["tangential"]]
    cam.thin_prism_coeffs[:] = [float(v) for v in view["thin_prism"]]
    cam.max_angle = float(view["max_angle"])
    cam.pose_start[:] = [float(v) for v in view["tq"]]
    cam.pose_end[:] = [float(v) for v in view["tq"]]
    if moving:
        cam.pose_end[0] = float(view["tq"][0]) + 0.01
    cam.timestamp_start_us, cam.timestamp_end_us = 0, 1
    return cam


def _device_views(views, colours=True, origins=True):
    out = []
    for v in views:
        out.append(dict(camera=_camera(v), distance=torch.as_tensor(v["distance"], device=DEV).contiguous(),
                        rgba=torch.as_tensor(v["rgba"], device=DEV).contiguous() if colours else None,
                        ray_origin=torch.as_tensor(v["ray_origin"], device=DEV).contiguous() if origins and v["ray_origin"] is not None else None))
    return out


def _volume(case, colours=True):
    return mesh.TSDFVolume(case["origin"], case["voxel"], case["dims"], case["truncation"], colours=colours, device=DEV)


def _state(vol):
    torch.cuda.synchronize()
    return {k: getattr(vol, k).cpu().numpy().astype(np.int64) for k in STATE if getattr(vol, k) is not None}


def _same_bytes(a, b):
    return all((getattr(a, k) is None and getattr(b, k) is None) or torch.equal(getattr(a, k), getattr(b, k)) for k in STATE)


@pytest.mark.parametrize("colours,origins", [(True, True), (False, False)])
@pytest.mark.parametrize("size,dims", mr.CASES)
def test_integration_against_the_reference(size, dims, colours, origins):
    """Calm voxels: cnt equal, acc within ACC_BAR x cnt quanta (the measured float32 band x K_BAND, tests/mesh_reference.py); near
    voxels: cnt within the number of views that made them near; colour sums within one unit per counted view where the colour's own
    threshold is not near either."""
    case = mr.sphere_case(size, dims)
    ref = mr.sphere_reference(size, dims, colours=colours, origins=origins)
    vol = _volume(case, colours).integrate(_device_views(case["views"], colours, origins))
    got = _state(vol)
    assert vol.n_views == len(case["views"])
    calm, near = ~ref["near"], ref["near"]
    d_acc, d_cnt = np.abs(got["acc"] - ref["acc"]), np.abs(got["cnt"] - ref["cnt"])
    print(f"[tsdf {size} {dims} colours={colours} origins={origins}] {int(ref['updated'].sum())} updated voxels, {int(near.sum())} near; calm: "
          f"cnt differs on {int((d_cnt[calm] > 0).sum())}, acc by at most {int(d_acc[calm].max())} quanta "
          f"(worst over its bar {float((d_acc[calm] / np.maximum(mr.ACC_BAR * ref['cnt'][calm], 1)).max()):.3f}); near: cnt differs on {int((d_cnt[near] > 0).sum())}")
    assert int(d_cnt[calm].max()) == 0
    assert bool((d_acc[calm] <= mr.ACC_BAR * ref["cnt"][calm]).all())
    assert bool((d_cnt[near] <= ref["near_views"][near]).all())
    assert bool((got["cnt"] >= 0).all()) and bool((np.abs(got["acc"]) <= 65536 * got["cnt"]).all())
    if colours:
        quiet = calm & ~ref["near_colour"]
        d_rgb = np.abs(got["rgb_sum"] - ref["rgb_sum"]).max(-1)
        print(f"[tsdf {size} {dims}] colours: rgb_cnt differs on {int((got['rgb_cnt'] != ref['rgb_cnt'])[quiet].sum())} quiet voxels, rgb_sum by at most {int(d_rgb[quiet].max())}")
        assert bool((got["rgb_cnt"] == ref["rgb_cnt"])[quiet].all()) and bool((d_rgb[quiet] <= ref["rgb_cnt"][quiet]).all())
        assert bool((got["rgb_cnt"] <= got["cnt"]).all()) and int(got["rgb_cnt"].max()) > 0
    else:
        assert vol.rgb_sum is None and vol.rgb_cnt is None
    tsdf = vol.tsdf().cpu().numpy()
    assert bool((np.isnan(tsdf) == (got["cnt"] == 0)).all()) and float(np.nanmax(np.abs(tsdf))) <= 1.0


@pytest.mark.parametrize("size,dims", [(16, (21, 17, 9)), (16, None)])
def test_exact_properties(size, dims):
    """One view a launch, batches of three, eight and two (what integrate() does with ten), and the reverse order give identical
    bytes; so do two runs; a view wholly outside the box changes no byte; a state filled by one view plus a second view equals both
    in one launch.  X = 21 is no multiple of 64 and the grid is not a cube."""
    case = mr.sphere_case(size, dims)
    views = _device_views(case["views"])
    whole = _volume(case).integrate(views)
    assert whole.n_views == 10 and int(whole.cnt.max()) > 1
    again = _volume(case).integrate(views)
    singles = _volume(case)
    for v in views:
        singles.integrate([v])
    threes = _volume(case)
    for at in range(0, len(views), 3):
        threes.integrate(views[at:at + 3])
    backwards = _volume(case).integrate(views[::-1])
    eight = _volume(case).integrate(views[:_capi.TSDF_MAX_VIEWS])
    eight.integrate(views[_capi.TSDF_MAX_VIEWS:])
    torch.cuda.synchronize()
    for other, what in ((again, "a second run"), (singles, "one view a launch"), (threes, "batches of three"), (backwards, "the reverse order"),
                        (eight, "eight and two")):
        assert _same_bytes(whole, other), what
    # a camera that looks away from the box: every voxel is behind it
    eye = np.asarray(mr._eye(17.3, 31.1))
    away = mr.make_camera("pinhole", 48, 40, tuple(eye), 1.2 * 48, target=tuple(2.0 * eye))
    away.update(distance=case["views"][0]["distance"], rgba=case["views"][0]["rgba"], ray_origin=None)
    before = {k: getattr(whole, k).clone() for k in STATE}
    whole.integrate(_device_views([away]))
    torch.cuda.synchronize()
    assert whole.n_views == 11 and all(torch.equal(before[k], getattr(whole, k)) for k in STATE), "a view that sees none of the box wrote"
    # the reference agrees that it sees nothing
    assert int(mr.integrate_views(case, [away])["cnt"].sum()) == 0
    first = _volume(case).integrate(views[:1])
    assert int(first.cnt.max()) == 1
    first.integrate(views[1:2])
    both = _volume(case).integrate(views[:2])
    torch.cuda.synchronize()
    assert _same_bytes(first, both) and int(both.cnt.max()) == 2


def _upload(case, ref, colours=True):
    vol = _volume(case, colours)
    for k in STATE:
        if getattr(vol, k) is not None:
            getattr(vol, k).copy_(torch.as_tensor(np.ascontiguousarray(ref[k]).astype(np.int32)))
    return vol


def _compare_meshes(got, want, voxel, label):
    v, c, f = (t.cpu().numpy() for t in got)
    rv, rc, rf = want
    assert v.dtype == np.float32 and c.dtype == np.float32 and f.dtype == np.int32
    assert v.shape == rv.shape and f.shape == rf.shape, f"{label}: {v.shape} vertices and {f.shape} faces, the reference {rv.shape} and {rf.shape}"
    assert np.array_equal(f, rf), f"{label}: the faces differ"
    bound = 1e-5 * voxel + 2.0 ** -21 * np.abs(rv)
    worst_v = float((np.abs(v - rv) / bound).max()) if len(v) else 0.0
    worst_c = float(np.abs(c - rc).max()) if len(v) else 0.0
    print(f"[surface nets {label}] {len(v)} vertices, {len(f)} faces; vertices at most {worst_v:.3f} of their bound off, colours {worst_c:.2e}")
    assert worst_v <= 1.0 and worst_c <= 1e-6


@pytest.mark.parametrize("size,dims", mr.CASES)
def test_extraction_against_the_reference_on_the_same_grid(size, dims):
    """Fed the reference's integer grid, the device's faces ARE the reference's; vertices within 1e-5 voxel + 2^-21 |coordinate| (a
    bound: the two values of a crossing have opposite sides, t = f0 / (f0 - f1) has no cancellation); colours within 1e-6."""
    case, ref = mr.sphere_case(size, dims), mr.sphere_reference(size, dims)
    want = mr.extract(ref["acc"], ref["cnt"], ref["rgb_sum"], ref["rgb_cnt"], case["origin"], case["voxel"])
    assert len(want[0]) > 100
    _compare_meshes(_upload(case, ref).extract(), want, case["voxel"], f"{size} {dims}")
    grey = mr.extract(ref["acc"], ref["cnt"], None, None, case["origin"], case["voxel"])
    _compare_meshes(_upload(case, ref, colours=False).extract(), grey, case["voxel"], f"{size} {dims} without colours")


def test_extraction_edge_cases():
    """An empty grid and a grid without a sign change give V = F = 0; min_count = 2 drops what one view alone saw; extraction twice
    gives the same bytes and leaves the state alone."""
    case = mr.sphere_case(16)
    empty = _volume(case)
    for vol in (empty, ):
        v, c, f = vol.extract()
        assert tuple(v.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    flat = _volume(case)
    flat.acc.fill_(40000)
    flat.cnt.fill_(1)
    assert [int(t.shape[0]) for t in flat.extract()] == [0, 0, 0]
    flat.acc.fill_(-40000)
    assert [int(t.shape[0]) for t in flat.extract()] == [0, 0, 0]
    two = mr.integrate_views(case, case["views"][:2])
    vol = _upload(case, two)
    before = {k: getattr(vol, k).clone() for k in STATE}
    one_view, both_views = vol.extract(min_count=1), vol.extract(min_count=2)
    _compare_meshes(one_view, mr.extract(two["acc"], two["cnt"], two["rgb_sum"], two["rgb_cnt"], case["origin"], case["voxel"], 1), case["voxel"], "two views, min_count 1")
    _compare_meshes(both_views, mr.extract(two["acc"], two["cnt"], two["rgb_sum"], two["rgb_cnt"], case["origin"], case["voxel"], 2), case["voxel"], "two views, min_count 2")
    assert 0 < both_views[0].shape[0] < one_view[0].shape[0] and both_views[2].shape[0] < one_view[2].shape[0]
    assert [int(t.shape[0]) for t in vol.extract(min_count=3)] == [0, 0, 0]
    again = vol.extract(min_count=1)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(one_view, again))
    assert all(torch.equal(before[k], getattr(vol, k)) for k in STATE)
    with pytest.raises(ValueError):
        vol.extract(min_count=0)


@pytest.mark.parametrize("size", mr.SPHERE_SIZES)
def test_the_sphere_end_to_end_on_the_device(size):
    """The device's own integration, then its extraction: closed, oriented, within one voxel edge of the unit sphere — the assertions
    the reference's mesh holds in tests/test_cpu_mesh.py."""
    case = mr.sphere_case(size)
    vol = _volume(case).integrate(_device_views(case["views"]))
    v, c, f = (t.cpu().numpy() for t in vol.extract())
    mr.check_closed_sphere(mr.mesh_report(v, f, case["voxel"]), f"device {size}^3")
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    want = np.clip(0.5 + 0.6 * v / np.linalg.norm(v, axis=1, keepdims=True), 0.0, 1.0)
    assert float(np.abs(c - want).max()) <= 0.15


def test_the_wall_through_the_renderer():
    """fuse_mesh over the three wall views of tests/surface_reference.py: every vertex within the bound the wall's points are held to
    (the reference's largest |z| + COLOUR_TOL x the largest distance) plus half a voxel; faces exist and face the cameras (z < 0)."""
    ref = sr.wall_points()
    model = native.NativeGaussianModel(sr.wall_scene(), device=DEV)
    renderer = surface.SurfaceRenderer(model, gut.Tracer({"render": {}}))
    batches = [to_batch(view, DEV) for view in sr.wall_views()]
    voxel = 0.05
    vol = mesh.volume_for(model, voxel=voxel, bounds=((-1.5, -1.2, -0.25), (1.5, 1.2, 0.25)), truncation_voxels=4, device=DEV)
    assert vol.dims == (60, 48, 10)
    assert mesh.fuse_mesh(renderer, batches, vol) is vol and vol.n_views == 3
    v, c, f = (t.cpu().numpy() for t in vol.extract())
    bound = ref["max_abs_z"] + COLOUR_TOL * ref["max_distance"] + 0.5 * voxel
    worst = float(np.abs(v[:, 2]).max())
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    print(f"[mesh wall] {len(v)} vertices, {len(f)} faces, largest |z| {worst:.5f}, bound {bound:.5f}; {int((normal[:, 2] >= 0).sum())} faces look away")
    assert len(f) > 0 and np.isfinite(v).all() and worst <= bound
    assert bool((normal[:, 2] < 0).all())
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0 and float(c.std()) > 0.0
    # the same call twice gives the same bytes; a view of a pinhole batch passes no origin plane
    again = mesh.fuse_mesh(renderer, batches, mesh.volume_for(model, voxel=voxel, bounds=((-1.5, -1.2, -0.25), (1.5, 1.2, 0.25)), device=DEV))
    torch.cuda.synchronize()
    assert _same_bytes(vol, again)
    assert mesh.view_of(batches[0], renderer.render(batches[0]))["ray_origin"] is None


def test_refusals_write_nothing_and_leave_later_calls_working():
    case = mr.sphere_case(16)
    views = _device_views(case["views"][:2])
    vol = _volume(case)
    lib = _capi.load()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def records(vs):
        rec = (_capi.GutTsdfView * max(1, len(vs)))()
        for r, v in zip(rec, vs):
            H, W = v["distance"].shape
            r.camera, r.width, r.height = C.pointer(v["camera"]), W, H
            r.d_distance, r.d_rgba = v["distance"].data_ptr(), v["rgba"].data_ptr()
            r.d_ray_origin = None if v["ray_origin"] is None else v["ray_origin"].data_ptr()
        return rec

    def refused(pattern, grid, n, rec):
        with pytest.raises(RuntimeError, match=pattern):
            _capi.check(lib.gut_tsdf_integrate(stream, None if grid is None else C.byref(grid), n, rec), "tsdf_integrate")
        torch.cuda.synchronize()
        assert not any(bool(getattr(vol, k).any()) for k in STATE), f"{pattern!r}: the refused call wrote"

    good = records(views)
    moving = [dict(views[0], camera=_camera(case["views"][0], moving=True))]
    refused("start and end poses differ", vol._grid(), 1, records(moving))
    refused(re.escape("n_views must be 1 .. 8, got 0"), vol._grid(), 0, good)
    refused(re.escape("n_views must be 1 .. 8, got 9"), vol._grid(), 9, (_capi.GutTsdfView * 9)())
    refused("null views", vol._grid(), 1, None)
    refused("null grid", None, 1, good)
    for field, pattern in (("d_distance", "null d_distance"), ("camera", "null camera")):
        rec = records(views)
        setattr(rec[1], field, None)
        refused(pattern, vol._grid(), 2, rec)
    for field in ("d_distance", "d_rgba", "d_ray_origin"):
        rec = records(views)
        setattr(rec[0], field, views[0]["distance"].data_ptr() + 2)
        refused("a plane is not 4-byte aligned", vol._grid(), 1, rec)
    rec = records(views)
    rec[0].width = 0
    refused("width and height must be >= 1", vol._grid(), 1, rec)
    rec = records(views)
    odd = _camera(case["views"][0])
    odd.model = 7
    rec[0].camera = C.pointer(odd)
    refused("unsupported camera model 7", vol._grid(), 1, rec)
    for change, pattern in ((dict(voxel=0.0), "voxel edge"), (dict(voxel=float("nan")), "voxel edge"), (dict(truncation=-1.0), "truncation"),
                            (dict(truncation=float("inf")), "truncation"), (dict(dims=(16, 0, 16)), "dims must be >= 1"),
                            (dict(dims=(1024, 1024, 1025)), "exceed 2\\^30"), (dict(dims=(-4, 4, 4)), "dims must be >= 1"),
                            (dict(d_acc=None), "null d_acc or d_cnt"), (dict(d_cnt=None), "null d_acc or d_cnt"),
                            (dict(d_rgb_cnt=None), "come together"), (dict(d_acc=vol.acc.data_ptr() + 1), "state pointer is not 4-byte aligned"),
                            (dict(d_rgb_sum=vol.rgb_sum.data_ptr() + 2), "state pointer is not 4-byte aligned")):
        grid = vol._grid()
        for k, val in change.items():
            if k == "dims":
                grid.dims[:] = val
            else:
                setattr(grid, k, val)
        refused(pattern, grid, 2, good)
    # the extraction's entry points refuse the same grids, and their own arguments
    n = vol.acc.numel()
    cell, quads = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    off = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.zeros((8, 3), device=DEV)
    faces = torch.zeros((8, 3), dtype=torch.int32, device=DEV)
    for rc in (lib.gut_surface_nets_count(stream, C.byref(vol._grid()), 0, cell.data_ptr(), quads.data_ptr()),
               lib.gut_surface_nets_count(stream, C.byref(vol._grid()), 1, None, quads.data_ptr()),
               lib.gut_surface_nets_count(stream, None, 1, cell.data_ptr(), quads.data_ptr()),
               lib.gut_surface_nets_emit(stream, C.byref(vol._grid()), 1, cell.data_ptr(), quads.data_ptr(), off.data_ptr(), off.data_ptr(),
                                         out.data_ptr(), None, faces.data_ptr()),
               lib.gut_surface_nets_emit(stream, C.byref(vol._grid()), 1, cell.data_ptr(), quads.data_ptr(), off.data_ptr() + 2, off.data_ptr(),
                                         out.data_ptr(), out.data_ptr(), faces.data_ptr())):
        assert rc != 0 and _capi.load().gut_last_error()
    torch.cuda.synchronize()
    assert not bool(cell.any()) and not bool(quads.any()) and not bool(out.any()) and not bool(faces.any())
    # the Python side
    with pytest.raises(ValueError, match="camera must be"):
        vol.integrate([dict(views[0], camera=None)])
    with pytest.raises(ValueError, match="distance must be"):
        vol.integrate([dict(views[0], distance=views[0]["distance"].double())])
    with pytest.raises(ValueError, match="rgba must be"):
        vol.integrate([dict(views[0], rgba=views[0]["rgba"][:, :, :3])])
    assert vol.n_views == 0 and not any(bool(getattr(vol, k).any()) for k in STATE)
    # and the volume still integrates what an untouched one does
    fresh = _volume(case).integrate(views)
    vol.integrate(views)
    torch.cuda.synchronize()
    assert _same_bytes(vol, fresh) and int(vol.cnt.max()) == 2


def test_trainer_exports_a_mesh(tmp_path, capsys):
    """--export-mesh on a small synthetic COLMAP scene: 8 views of 96 x 96 (7 to train on, 1 held out), 40 iterations, 32 voxels along
    the longest edge.  A readable mesh.ply and the mesh_* keys; without the flag neither; the refusals at configuration time."""
    from tests.synthetic_colmap import write_synthetic_colmap
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=8, size=96, n_teacher=20_000, n_points=2_000)
    out = str(tmp_path / "run")
    assert trainer_mod.main(["--path", root, "--n-iterations", "40", "--out-dir", out, "--export-mesh", "--mesh-resolution", "32"]) == 0
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    print(f"[trainer mesh] {stats['mesh_vertices']} vertices, {stats['mesh_faces']} faces from {stats['mesh_views']} views, voxel {stats['mesh_voxel']:.4f}, dims {stats['mesh_dims']}")
    assert stats["mesh_views"] == 7 and stats["mesh_voxel"] > 0.0 and len(stats["mesh_dims"]) == 3 and max(stats["mesh_dims"]) == 32
    assert stats["mesh_vertices"] >= 0 and stats["mesh_faces"] >= 0 and stats["mesh_faces"] % 2 == 0
    got = io_ply.read_ply(os.path.join(out, "mesh.ply"))
    assert got["positions"].shape == (stats["mesh_vertices"], 3) and got["rgb"].shape == (stats["mesh_vertices"], 3)
    assert got["faces"].shape == (stats["mesh_faces"], 3) and np.isfinite(got["positions"]).all()
    assert stats["mesh_faces"] == 0 or (int(got["faces"].min()) >= 0 and int(got["faces"].max()) < stats["mesh_vertices"])
    assert not any(k.startswith("points") for k in stats) and not os.path.exists(os.path.join(out, "points.ply"))
    out2 = str(tmp_path / "plain")
    assert trainer_mod.main(["--path", root, "--n-iterations", "5", "--out-dir", out2]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["stats"]
    assert not any(k.startswith("mesh") for k in plain) and not os.path.exists(os.path.join(out2, "mesh.ply"))
    with pytest.raises(ValueError, match="mesh: the mesh export needs the unsorted variant"):
        trainer_mod.resolve_config({"mesh": {"enabled": True}, "render": {"splat": {"k_buffer_size": 8}}})
    with pytest.raises(ValueError, match="mesh: the mesh export needs render.particle_kernel_degree 2"):
        trainer_mod.resolve_config({"mesh": {"enabled": True}, "render": {"particle_kernel_degree": 3}})
    from tests.test_cpu_trainer import _FakeStepper, _model, _trainer
    st = _FakeStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError, match="mesh: data-parallel"):
        _trainer(dict(n_iterations=1, mesh=dict(enabled=True)), stepper=st)
