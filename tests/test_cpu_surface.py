"""The surface walk without a GPU: the CPU reference earns its hit-distance formula against the oracle's own distance
plane, the near sets of the device test fit their cap on the reference alone, the single-tile case carries its state across chunks,
the wall's reference points lie on the wall; the host logic of 3dgrut_amd/surface.py, the point-cloud PLY, the trainer's `points`
block and the binding."""
import importlib

import numpy as np
import pytest
import torch

from tests import contribution_reference as cr
from tests import surface_reference as sr
from tests.common import COLOUR_TOL, to_batch

capi = importlib.import_module("3dgrut_amd._capi")
io_ply = importlib.import_module("3dgrut_amd.io_ply")
surface = importlib.import_module("3dgrut_amd.surface")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")

MODES = tuple(("level", lv) for lv in sr.LEVELS) + (("max_weight", None),)


def _planes(name, mode, level):
    return sr.level_planes(name, level) if mode == "level" else sr.max_weight_planes(name)


@pytest.mark.parametrize("name", cr.CASES)
def test_the_hit_distance_formula_reproduces_the_oracles_distance_plane(name):
    """oracle.debug_ray does not return hit_t, so the reference recomputes it from d12, c2w and the ray; sum of w * hit_t per pixel
    must be the oracle's own `dist` plane, at the bar check_colour_outliers holds that plane to: COLOUR_TOL relative to
    max(1, largest distance).  Measured: the largest absolute difference over the four cases is 1.2e-6, 2.7e-7 of the largest distance."""
    s = sr.surface_case(name)
    ref = s["fwd"]["dist"].reshape(s["H"], s["W"]).astype(np.float64)
    worst, far = float(np.abs(s["dist_sum"] - ref).max()), float(np.abs(ref).max())
    print(f"[surface reference {name}] sum w hit_t vs the oracle's dist: worst {worst:.3e}, largest distance {far:.4f}, "
          f"{int(s['hit'].sum())} pixels with a hit")
    assert worst / max(1.0, far) <= COLOUR_TOL
    assert far > 1.0 and int(s["hit"].sum()) > 100


@pytest.mark.parametrize("name", cr.CASES)
def test_reference_planes_and_the_cap_of_the_near_sets(name):
    """In every case, mode and level the near set — the pixels at which the device may choose differently — is at most 5 % of the
    pixels that composited anything.  The planes themselves: a chosen entry is one of the pixel's own, level planes are nested (a
    lower level is crossed later or never), the largest weight is at least the level entry's."""
    s = sr.surface_case(name)
    hit = int(s["hit"].sum())
    for mode, level in MODES:
        p = _planes(name, mode, level)
        near = int((p["near"] & s["hit"]).sum())
        print(f"[surface reference {name}] {mode} {level}: {near} near of {hit} pixels with a hit, {int((p['id'] >= 0).sum())} with an id")
        assert near <= 0.05 * hit
        assert not bool((p["id"] >= 0)[~s["hit"]].any())
        assert bool(((p["distance"] > 0) == (p["id"] >= 0)).all()) and bool(((p["weight"] > 0) == (p["id"] >= 0)).all())
        for q, (e_ids, *_rest) in enumerate(s["entries"]):
            got = int(p["id"].reshape(-1)[q])
            assert got == -1 or got in e_ids
    half, tenth, most = (sr.level_planes(name, lv) for lv in (0.5, 0.1, 0.9))
    top = sr.max_weight_planes(name)
    assert bool(((tenth["id"] >= 0) <= (half["id"] >= 0)).all()) and bool(((half["id"] >= 0) <= (most["id"] >= 0)).all())
    both = (tenth["id"] >= 0)
    assert bool((tenth["position"][both] >= half["position"][both]).all()) and bool((half["position"][both] >= most["position"][both]).all())
    assert bool(((top["id"] >= 0) == s["hit"]).all())
    assert bool((top["weight"] >= half["weight"]).all())


def test_the_single_tile_case_crosses_behind_the_first_chunk():
    """single_tile_1025 at level 0.9 is the case of the state carried across the 256-entry chunks: measured, 62 of its 84 crossing
    pixels cross at list position >= 256.  At level 0.1 nothing crosses there: the all-none plane."""
    most = sr.level_planes("single_tile_1025", 0.9)
    crossing = most["id"] >= 0
    late = int((most["position"][crossing] >= 256).sum())
    print(f"[surface reference single_tile_1025] level 0.9: {int(crossing.sum())} crossing pixels, {late} at list position >= 256")
    assert late >= 32
    tenth = sr.level_planes("single_tile_1025", 0.1)
    assert not bool((tenth["id"] >= 0).any()) and not bool(tenth["distance"].any()) and not bool(tenth["weight"].any())


def test_the_walls_reference_points_lie_on_the_wall():
    """The reference's level-0.5 points of the three wall views and their largest |z| (printed; DESIGN.md §18 records it).  A hit
    point is where the ray is closest to the Gaussian's centre in the Gaussian's own metric, and an accepted one lies inside the 3
    sigma ellipsoid (the response cut): its |z| is at most that ellipsoid's extent along z, 3 |(s R^T) e_z|, at most over the discs."""
    w = sr.wall_points()
    sc = sr.wall_scene()
    R = sr.quat_rotation(sc["rotation"])
    extent = 3.0 * np.linalg.norm(R[:, 2, :] * sc["scale"].astype(np.float64), axis=1) + np.abs(sc["positions"][:, 2])
    print(f"[surface wall] {w['points'].shape[0]} reference points, largest |z| {w['max_abs_z']:.6f} (3 sigma extent of the discs "
          f"along z: {float(extent.max()):.6f}), largest distance {w['max_distance']:.4f}")
    assert w["points"].shape[0] > 3000 and np.isfinite(w["points"]).all()
    assert w["max_abs_z"] <= float(extent.max())
    assert 200 <= sc["positions"].shape[0] <= 400 and len(sr.wall_views()) == 3


def test_backproject_against_float64():
    """surface.backproject on the reference distances of the ragged case against the float64 c2w arithmetic: 1e-5 relative to the
    largest coordinate, a float32 matrix-vector product's bar; a distance of 0 gives NaN."""
    s = sr.surface_case("ragged_70x45")
    dist = sr.level_planes("ragged_70x45", 0.5)["distance"]
    want = sr.backproject(s["view"], dist)
    got = surface.backproject(to_batch(s["view"], "cpu"), torch.as_tensor(dist)).numpy()
    assert got.shape == (s["H"], s["W"], 3) and got.dtype == np.float32
    some = dist > 0
    assert bool(np.isnan(got[~some]).all()) and bool(np.isnan(want[~some]).all()) and int(some.sum()) > 1000
    worst = float(np.abs(got[some] - want[some]).max() / np.abs(want[some]).max())
    print(f"[surface backproject] worst relative difference {worst:.3e}")
    assert worst <= 1e-5


def test_first_per_voxel_keeps_the_first_point_of_every_cell():
    xyz = torch.tensor([[0.1, 0.1, 0.1], [1.2, 0.0, 0.0], [0.4, 0.4, 0.4], [-0.1, 0.0, 0.0], [1.9, 0.9, 0.9], [-0.9, 0.5, 0.5]])
    assert surface.first_per_voxel(xyz, 1.0).tolist() == [0, 1, 3]
    assert surface.first_per_voxel(xyz, 0.25).tolist() == [0, 1, 2, 3, 4, 5]
    assert surface.first_per_voxel(xyz, 100.0).tolist() == [0, 3]


def test_point_cloud_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(37, 3)).astype(np.float32)
    rgb = rng.uniform(-0.2, 1.2, (37, 3)).astype(np.float32)
    path = str(tmp_path / "points.ply")
    io_ply.write_point_cloud(path, xyz, rgb)
    back = io_ply.read_ply(path)
    assert sorted(back) == ["positions", "rgb"]
    assert np.array_equal(back["positions"], xyz) and back["rgb"].dtype == np.uint8
    assert np.array_equal(back["rgb"], np.rint(np.clip(rgb, 0, 1) * 255).astype(np.uint8))
    with open(path, "rb") as fh:
        head = fh.read(200).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n") and "property uchar blue\nend_header\n" in head
    io_ply.write_point_cloud(path, np.zeros((0, 3)), np.zeros((0, 3)))
    assert io_ply.read_ply(path)["positions"].shape == (0, 3)
    with pytest.raises(ValueError):
        io_ply.write_point_cloud(path, xyz, rgb[:5])
    # a Gaussian PLY still reads as one
    io_ply.write_ply(path, xyz, np.zeros((37, 1)), np.ones((37, 4)), np.zeros((37, 3)), np.zeros((37, 48)))
    assert "features48" in io_ply.read_ply(path)


def test_points_config_and_command_line():
    conf = trainer_mod.resolve_config({})
    assert conf["points"] == dict(enabled=False, level=0.5, stride=1, voxel=0.0) == surface.DEFAULTS
    for bad in (dict(level=0.0), dict(level=1.0), dict(level=float("nan")), dict(level="0.5"), dict(stride=0), dict(stride=1.5), dict(stride=True),
                dict(voxel=-1.0), dict(voxel=float("inf")), dict(enabled=1), dict(unknown=1)):
        with pytest.raises(ValueError, match="points"):
            trainer_mod.resolve_config({"points": bad})
    ap = trainer_mod.build_parser()
    off = trainer_mod.config_from_args(ap.parse_args(["--path", "x"]))
    assert off["points"] == surface.DEFAULTS
    on = trainer_mod.config_from_args(ap.parse_args(["--path", "x", "--export-points", "--points-level", "0.4", "--points-stride", "2",
                                                      "--points-voxel", "0.05"]))
    assert on["points"] == dict(enabled=True, level=0.4, stride=2, voxel=0.05)
    trainer_mod.resolve_config(on)


def test_binding():
    lib = capi.load()
    assert "gut_trace_surface" in capi.EXPORTS and hasattr(lib, "gut_trace_surface")
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    assert len(lib.gut_trace_surface.argtypes) == 16
    assert (capi.SURFACE_LEVEL, capi.SURFACE_MAX_WEIGHT) == (0, 1)
    assert int(lib.gut_abi_version()) == 6
