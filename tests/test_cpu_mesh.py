"""The mesh export without a GPU: the reference's near sets fit their cap and its float32 band gives the device's bar;
the reference's own sphere is closed, oriented and within a voxel of the unit sphere at 16^3, 24^3 and 32^3; the host logic of
3dgrut_amd/mesh.py, the mesh PLY, the trainer's `mesh` block and the binding."""
import importlib
import inspect
import types

import numpy as np
import pytest
import torch

from tests import mesh_reference as mr
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

capi = importlib.import_module("3dgrut_amd._capi")
io_ply = importlib.import_module("3dgrut_amd.io_ply")
mesh = importlib.import_module("3dgrut_amd.mesh")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")


@pytest.mark.parametrize("size,dims", mr.CASES)
def test_the_near_sets_fit_their_cap(size, dims):
    """The near voxels — those at which another valid fp32 evaluation may take another pixel or another side of a threshold — are at
    most 5 % of the voxels some view updated, in every case; with and without the origin planes."""
    for origins in (True, False):
        ref = mr.sphere_reference(size, dims, origins=origins)
        updated, near = int(ref["updated"].sum()), int((ref["near"] & ref["updated"]).sum())
        print(f"[mesh reference {size} {dims} origins={origins}] {near} near of {updated} updated voxels ({near / updated:.4f}), "
              f"{int(ref['near_colour'].sum())} at the colour's threshold")
        assert updated > 0.5 * ref["updated"].size and near <= mr.NEAR_CAP * updated
        assert int(ref["cnt"].max()) <= len(mr.sphere_views()) and int(ref["near_views"].max()) <= len(mr.sphere_views())
        assert bool((ref["rgb_cnt"] <= ref["cnt"]).all()) and int(ref["rgb_cnt"].max()) > 0
        assert bool((ref["rgb_sum"] <= 255 * ref["rgb_cnt"][..., None]).all()) and bool((np.abs(ref["acc"]) <= 65536 * ref["cnt"]).all())


def test_the_float32_band_gives_the_bar():
    """ACC_BAR is K_BAND x the largest |acc32 - acc64| of a calm voxel over the cases, and cnt agrees on every calm voxel.  Measured:
    1, 1, 2 and 1 quanta on the four cases, 0 differing counts."""
    worst = 0
    for size, dims in mr.CASES:
        band, cnt_differs, calm = mr.float32_band(size, dims)
        print(f"[mesh reference {size} {dims}] float32 against float64 on {calm} calm voxels: acc differs by at most {band} quanta, cnt on {cnt_differs}")
        assert cnt_differs == 0 and calm > 1000
        worst = max(worst, band)
    assert mr.ACC_BAR == mr.K_BAND * worst
    assert mr.ACC_BAR < 10.0


@pytest.mark.parametrize("size", mr.SPHERE_SIZES)
def test_the_references_sphere_is_closed_oriented_and_round(size):
    """No edge in exactly one triangle, every directed edge as often as its reverse, every normal away from the centre, V - E + F = 2
    where no edge has more than two triangles, every vertex within one voxel edge of the unit sphere.  Measured: 0.44, 0.48 and 0.55
    voxel, no crowded edge."""
    vertices, colours, faces = mr.sphere_mesh(size)
    mr.check_closed_sphere(mr.mesh_report(vertices, faces, mr.sphere_case(size)["voxel"]), f"reference {size}^3")
    assert colours.shape == vertices.shape and float(colours.min()) >= 0.0 and float(colours.max()) <= 1.0
    # the colour is 0.5 + 0.6 x the direction, clamped, in steps of 1 / 255, seen through pixels: loosely the direction's
    want = np.clip(0.5 + 0.6 * vertices / np.linalg.norm(vertices, axis=1, keepdims=True), 0.0, 1.0)
    assert float(np.abs(colours - want).max()) <= 0.15


def test_extraction_of_hand_made_grids():
    """An empty grid and a grid without a sign change give nothing; one inside voxel in a 3^3 grid gives the octahedron-like closed
    surface of its eight cells; min_count drops what too few views saw."""
    z = np.zeros((3, 3, 3), np.int64)
    for acc, cnt in ((z, z), (z + 5, z + 1), (z - 5, z + 1)):
        v, c, f = mr.extract(acc, cnt, None, None, (0, 0, 0), 1.0)
        assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    acc, cnt = z + 30000, z + 1
    acc[1, 1, 1] = -30000
    v, c, f = mr.extract(acc, cnt, None, None, (0.0, 0.0, 0.0), 1.0)
    rep = mr.mesh_report(v, f, 1.0, centre=(1.5, 1.5, 1.5), radius=0.5)
    assert rep["V"] == 8 and rep["F"] == 12 and rep["boundary_edges"] == 0 and rep["unbalanced_edges"] == 0 and rep["inward"] == 0 and rep["euler"] == 2
    assert np.allclose(np.abs(v - 1.5), 1.0 / 6.0) and bool((c == 0.5).all())       # three crossings of 1/2 a cell, averaged with the corner
    cnt2 = cnt.copy()
    cnt2[0, 0, 0] = 0                                                                # one unobserved corner: its cell and its quads go
    v2, _, f2 = mr.extract(acc, cnt2, None, None, (0.0, 0.0, 0.0), 1.0)
    assert len(v2) == 7 and len(f2) == 12 - 6
    assert len(mr.extract(acc, cnt, None, None, (0, 0, 0), 1.0, min_count=2)[0]) == 0


def test_check_config_accepts_and_refuses():
    ok = dict(mesh.DEFAULTS)
    assert mesh.check_config(ok) is ok and ok["enabled"] is False
    for good in (dict(enabled=True), dict(voxel=0.01), dict(bounds=((-1, -1, -1), (1, 2, 3))), dict(bounds=[[0, 0, 0], [1, 1, 1]]),
                 dict(resolution=10, truncation_voxels=4), dict(truncation_voxels=2.5), dict(min_count=3), dict(level=0.3)):
        mesh.check_config(dict(mesh.DEFAULTS, **good))
    for bad in (dict(enabled="yes"), dict(level=0.0), dict(level=1.0), dict(level="0.5"), dict(resolution=9), dict(resolution=64.0),
                dict(resolution=True), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel="0.1"),
                dict(truncation_voxels=0), dict(truncation_voxels=float("inf")), dict(min_count=0), dict(min_count=1.5), dict(min_count=True),
                dict(bounds=((0, 0, 0), (1, 1))), dict(bounds=((0, 0, 0), (1, 0, 1))), dict(bounds="box"), dict(bounds=((0, 0, 0), (1, 1, float("inf")))),
                dict(colour=True)):
        with pytest.raises(ValueError):
            mesh.check_config(dict(mesh.DEFAULTS, **bad))


def test_volume_for_sizes():
    """The quantile box grown by the truncation is `resolution` voxels along its longest edge; a given voxel or box is taken as it is."""
    rng = np.random.default_rng(3)
    pos = rng.uniform(-1.0, 1.0, (20001, 3)) * np.array([2.0, 1.0, 0.5])
    pos[:50] *= 40.0                                                # outliers the quantiles drop
    model = types.SimpleNamespace(positions=torch.as_tensor(pos, dtype=torch.float32))
    ordered = np.sort(pos.astype(np.float32), axis=0)
    lo, hi = ordered[200], ordered[19800]
    vol = mesh.volume_for(model, resolution=32, truncation_voxels=4, device="cpu")
    assert vol.voxel == pytest.approx((hi[0] - lo[0]) / 24.0, rel=1e-6) and vol.truncation == pytest.approx(4 * vol.voxel)
    assert vol.dims[0] == 32 and vol.dims == tuple(int(np.ceil((hi[a] - lo[a]) / vol.voxel + 8 - 1e-6)) for a in range(3))
    assert np.allclose(vol.origin, lo - 4 * vol.voxel, rtol=1e-6, atol=1e-6)
    assert tuple(vol.acc.shape) == vol.dims[::-1] and vol.acc.dtype == torch.int32 and tuple(vol.rgb_sum.shape) == vol.dims[::-1] + (3,)
    assert vol.n_views == 0 and int(vol.cnt.abs().sum()) == 0 and bool(torch.isnan(vol.tsdf()).all())
    fixed = mesh.volume_for(model, voxel=0.25, truncation_voxels=2, colours=False, device="cpu")
    assert fixed.voxel == 0.25 and fixed.truncation == 0.5 and fixed.rgb_sum is None and fixed.rgb_cnt is None
    assert fixed.dims == tuple(int(np.ceil((hi[a] - lo[a] + 1.0) / 0.25 - 1e-6)) for a in range(3))
    boxed = mesh.volume_for(model, resolution=20, bounds=((-1, -2, -3), (1, 2, 2)), device="cpu")
    assert boxed.origin == (-1.0, -2.0, -3.0) and boxed.voxel == 0.25 and boxed.dims == (8, 16, 20) and boxed.truncation == 1.0
    for bad in (dict(resolution=8), dict(voxel=0.0), dict(truncation_voxels=0.0), dict(voxel=1e-4)):
        with pytest.raises(ValueError):
            mesh.volume_for(model, device="cpu", **bad)
    with pytest.raises(ValueError):
        mesh.TSDFVolume((0, 0, 0), 0.1, (1024, 1024, 1025), 0.4, device="cpu")
    with pytest.raises(ValueError):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.0, device="cpu")
    small = mesh.TSDFVolume((0, 0, 0), 0.1, (4, 3, 2), 0.4, device="cpu")
    small.n_views = mesh.MAX_VIEWS
    with pytest.raises(ValueError, match="32767"):
        small.integrate([dict()])
    with pytest.raises(RuntimeError):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 3, 2), 0.4, device="cpu").extract()


def test_mesh_ply_round_trip(tmp_path):
    vertices, colours, faces = mr.sphere_mesh(16)
    path = str(tmp_path / "mesh.ply")
    io_ply.write_mesh(path, vertices, colours, faces)
    back = io_ply.read_ply(path)
    assert sorted(back) == ["faces", "positions", "rgb"]
    assert np.array_equal(back["positions"], vertices.astype(np.float32)) and back["faces"].dtype == np.int32 and np.array_equal(back["faces"], faces)
    assert back["rgb"].dtype == np.uint8 and np.array_equal(back["rgb"], np.rint(np.clip(colours.astype(np.float32), 0, 1) * 255.0).astype(np.uint8))
    header = open(path, "rb").read(400).decode("ascii", "replace")
    assert "element face %d" % len(faces) in header and "property list uchar int vertex_indices" in header
    empty = str(tmp_path / "empty.ply")
    io_ply.write_mesh(empty, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert io_ply.read_ply(empty)["faces"].shape == (0, 3)
    with pytest.raises(ValueError):
        io_ply.write_mesh(path, vertices, colours[:-1], faces)
    with pytest.raises(ValueError):
        io_ply.write_mesh(path, vertices, colours, faces + len(vertices))
    cloud = str(tmp_path / "points.ply")                      # a point cloud still reads as one
    io_ply.write_point_cloud(cloud, vertices, colours)
    assert sorted(io_ply.read_ply(cloud)) == ["positions", "rgb"]


def test_the_trainers_mesh_block():
    conf = trainer_mod.resolve_config({})
    assert conf["mesh"] == mesh.DEFAULTS and conf["mesh"] is not mesh.DEFAULTS
    on = trainer_mod.resolve_config({"mesh": {"enabled": True, "resolution": 64, "bounds": [[-1, -1, -1], [1, 1, 1]]}})
    assert on["mesh"]["enabled"] and on["mesh"]["resolution"] == 64 and on["mesh"]["truncation_voxels"] == 4 and on["mesh"]["voxel"] is None
    for bad in ({"mesh": {"resolution": 4}}, {"mesh": {"colour": True}}, {"mesh": {"enabled": True}, "render": {"splat": {"k_buffer_size": 8}}},
                {"mesh": {"enabled": True}, "render": {"particle_kernel_degree": 4}}):
        with pytest.raises(ValueError):
            trainer_mod.resolve_config(bad)
    trainer_mod.resolve_config({"mesh": {"enabled": False}, "render": {"splat": {"k_buffer_size": 8}}})      # refused only when asked for
    a = trainer_mod.build_parser().parse_args(["--path", "x", "--export-mesh", "--mesh-resolution", "96", "--mesh-voxel", "0.02"])
    c = trainer_mod.config_from_args(a)
    assert c["mesh"]["enabled"] is True and c["mesh"]["resolution"] == 96 and c["mesh"]["voxel"] == 0.02
    assert trainer_mod.config_from_args(trainer_mod.build_parser().parse_args(["--path", "x"]))["mesh"]["enabled"] is False
    st = _FakeStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError, match="mesh: data-parallel"):
        _trainer(dict(n_iterations=1, mesh=dict(enabled=True)), stepper=st)
    _trainer(dict(n_iterations=1, mesh=dict(enabled=True)))          # one GPU: accepted


def test_bindings_and_abi_version():
    assert capi.GUT_ABI_VERSION == 6 and capi.TSDF_MAX_VIEWS == 8
    for name in ("gut_tsdf_integrate", "gut_surface_nets_count", "gut_surface_nets_emit"):
        assert name in capi.EXPORTS
    import ctypes as C
    assert C.sizeof(capi.GutTsdfGrid) == 64 and C.sizeof(capi.GutTsdfView) == 40
    lib = capi.load()
    assert lib.gut_abi_version() == 6
    assert len(lib.gut_tsdf_integrate.argtypes) == 4 and len(lib.gut_surface_nets_count.argtypes) == 5 and len(lib.gut_surface_nets_emit.argtypes) == 10
    assert {"integrate", "tsdf", "extract"} <= set(dir(mesh.TSDFVolume)) and "min_count" in inspect.signature(mesh.TSDFVolume.extract).parameters
    assert list(inspect.signature(mesh.fuse_mesh).parameters) == ["renderer", "batches", "volume", "level"]
