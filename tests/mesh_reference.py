"""The CPU reference of the mesh export (gut_tsdf_integrate and the surface nets of gut_fuse.hip).

`integrate_views(grid, views)` restates the integration in float64 numpy, on the same float32 inputs the device gets (poses, intrinsics,
distance planes, colours, origin planes); with np.float32 it is the same statement rounded to float32 after every operation, the
band a legitimate fp32 evaluation may lie in.  `extract(...)` restates the surface nets on the INTEGER grid: which cells and edges
exist is exact by construction, only the vertex coordinates are floating point (float64 here).

The analytic case: a unit sphere at the origin inside an enclosing sphere of radius 6, so that every ray has a surface (without it
the voxels beside the silhouette that only grazing rays reach stay negative and a second component appears).  The distance planes are
ray-sphere intersections along the rays that the camera model's own projection inverts; no renderer is involved.  Ten views at
distance 3.5, 32 x 32 to 64 x 64: four on each of two elevations, staggered, one of them through a distorted pinhole and one through
a fisheye, one above, one below; two of them with rays that start off the sensor position (an origin plane).  The grid origin and the camera positions are in general position (irrational-looking offsets): with a
symmetric grid and on-axis cameras 13 to 15 % of the voxels project exactly onto pixel boundaries.

A voxel is NEAR if in some view (a) its projection lies within 1e-3 pixel of a pixel boundary or of the image border, (b)
|s + truncation| <= 1e-4 truncation, or (c) its sensor-frame depth or the projection's validity test is within 1e-4 of its threshold
(z against 0 in units of the truncation, the distortion factor against 0.8 and 1.2, the fisheye angle against max_angle).  Elsewhere —
CALM voxels — every evaluation takes the same pixel and the same side of every threshold, and differs by rounding alone.  The colour
has one more threshold, |s| <= truncation: `near_colour` marks |s - truncation| <= 1e-4 truncation.

ACC_BAR: 2.5 x the largest |acc32 - acc64| of a calm voxel over every case (2.5 is DESIGN.md §3's constant for fp32 bands, K_BAND of
tests/common.py).  Measured on this reference: 1 quantum at 16^3, 24^3 and 21 x 17 x 9, 2 quanta at 32^3, with cnt equal on every calm
voxel; so the bar is 5 quanta.  test_cpu_mesh.py re-measures it.
The device is held to ACC_BAR x the voxel's cnt.

Everything is computed once and cached: the tests share it and leave it unchanged."""
import functools
import importlib
import math

import numpy as np

from tests.common import K_BAND, cams, pose

ACC_BAR = 5.0          # quanta of 2^-16; K_BAND x the measured float32 band of 2 quanta
NEAR_PIXEL, NEAR_REL = 1e-3, 1e-4
NEAR_CAP = 0.05
SPHERE_SIZES = (16, 24, 32)
CASES = ((16, None), (24, None), (32, None), (16, (21, 17, 9)))     # (size, dims): the spheres, and a non-cubic box with 16's voxel
ENCLOSING_RADIUS = 6.0
CAMERA_DISTANCE = 3.5
TRUNCATION_VOXELS = 4.0
HALF_BOX = 1.3
FOCAL = 1.2             # focal length / image width: the sphere and its truncation band fill the images
ORIGIN_OFFSET = (0.0137, -0.0071, 0.0213)

DISTORTION = dict(radial=[-0.05, 0.012, -0.002, 0.004, -0.001, 0.0005], tangential=[0.0011, -0.0007], thin_prism=[0.0004, -0.0002, 0.0003, 0.0001])
FISHEYE_RADIAL = [-0.03, -0.006, 0.001, -0.0003]


# ---- cameras: the projection in any float type, and the rays that invert it ----
def quat_rows(tq, dtype):
    """(R [3,3], t [3]) of a [t(3), q(xyzw)] pose: gut_api.cpp's quat_to_rot, in `dtype`."""
    t = np.asarray(tq[:3], dtype)
    x, y, z, w = (dtype(v) for v in np.asarray(tq[3:7], dtype))
    one, two = dtype(1), dtype(2)
    R = np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                  [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                  [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype)
    return R, t


def project(view, c, dtype):
    """(u, v, valid, ok, margin, depth_margin) of sensor-frame points c [n,3] in `dtype`, operation by operation as project_pinhole /
    project_fisheye with tol = 0.  ok: valid but for the image rectangle.  margin: how far the distortion factor is from 0.8 and
    1.2, the fisheye angle from max_angle; depth_margin: |z| of a pinhole; inf where there is no such test."""
    T = dtype
    px, py, pz = c[:, 0], c[:, 1], c[:, 2]
    fl, pp = np.asarray(view["focal_length"], T), np.asarray(view["principal_point"], T)
    W, H = T(view["W"]), T(view["H"])
    with np.errstate(all="ignore"):
        if view["model"] == "pinhole":
            front = pz > 0
            rz = T(1) / pz
            un, vn = px * rz, py * rz
            depth_margin = np.abs(pz)
            if not view["distorted"]:
                u, v = un * fl[0] + pp[0], vn * fl[1] + pp[1]
                ok, margin = front, np.full(len(pz), np.inf)
            else:
                k, tg, tp = np.asarray(view["radial"], T), np.asarray(view["tangential"], T), np.asarray(view["thin_prism"], T)
                u2, v2 = un * un, vn * vn
                r2 = u2 + v2
                a1, a2, a3 = T(2) * un * vn, r2 + T(2) * u2, r2 + T(2) * v2
                num = T(1) + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
                den = T(1) + r2 * (k[3] + r2 * (k[4] + r2 * k[5]))
                icd = num / den
                dx = tg[0] * a1 + tg[1] * a2 + r2 * (tp[0] + r2 * tp[1])
                dy = tg[0] * a3 + tg[1] * a1 + r2 * (tp[2] + r2 * tp[3])
                xd, yd = icd * un + dx, icd * vn + dy
                radial_ok = (icd > T(0.8)) & (icd < T(1.2))
                u, v = xd * fl[0] + pp[0], yd * fl[1] + pp[1]
                ok = front & radial_ok
                margin = np.minimum(np.abs(icd.astype(np.float64) - 0.8), np.abs(icd.astype(np.float64) - 1.2))
        else:
            k = np.asarray(view["radial"], T)
            eps = T(1.1920929e-07)
            rho = np.maximum(np.sqrt(px * px + py * py), eps)
            theta_full = np.arctan2(rho, pz).astype(T)
            max_angle = T(view["max_angle"])
            theta = np.minimum(theta_full, max_angle)
            t2 = theta * theta
            poly = k[3]
            poly = t2 * poly + k[2]
            poly = t2 * poly + k[1]
            poly = t2 * poly + k[0]
            delta = (theta * (poly * t2 + T(1))) / rho
            u, v = fl[0] * px * delta + pp[0], fl[1] * py * delta + pp[1]
            ok = theta < max_angle
            margin = np.abs(theta_full.astype(np.float64) - float(max_angle))
            depth_margin = np.full(len(pz), np.inf)
        valid = ok & (u > 0) & (v > 0) & (u < W) & (v < H)
    return u, v, valid, ok, margin, depth_margin


def pixel_rays(view):
    """float64 unit directions [H,W,3] in the sensor frame through the pixel centres, inverting `project` (fixed-point iteration on
    the distortion, Newton on the fisheye polynomial)."""
    W, H = view["W"], view["H"]
    fl, pp = np.asarray(view["focal_length"], np.float64), np.asarray(view["principal_point"], np.float64)
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="xy")
    xd, yd = (x - pp[0]) / fl[0], (y - pp[1]) / fl[1]
    if view["model"] == "pinhole":
        un, vn = xd.copy(), yd.copy()
        if view["distorted"]:
            k, tg, tp = (np.asarray(view[n], np.float64) for n in ("radial", "tangential", "thin_prism"))
            for _ in range(60):
                r2 = un * un + vn * vn
                icd = (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) / (1 + r2 * (k[3] + r2 * (k[4] + r2 * k[5])))
                dx = tg[0] * 2 * un * vn + tg[1] * (r2 + 2 * un * un) + r2 * (tp[0] + r2 * tp[1])
                dy = tg[0] * (r2 + 2 * vn * vn) + tg[1] * 2 * un * vn + r2 * (tp[2] + r2 * tp[3])
                un, vn = (xd - dx) / icd, (yd - dy) / icd
        d = np.stack([un, vn, np.ones_like(un)], -1)
    else:
        k = np.asarray(view["radial"], np.float64)
        delta = np.sqrt(xd * xd + yd * yd)
        theta = delta.copy()
        for _ in range(30):
            t2 = theta * theta
            f = theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - delta
            df = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
            theta = theta - f / df
        s = np.sin(theta) / np.maximum(delta, 1e-12)
        d = np.stack([s * xd, s * yd, np.cos(theta)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def make_camera(model, W, H, eye, fx, distorted=False, target=(0.0, 0.0, 0.0)):
    c2w = cams.look_at_c2w(eye, target)
    tq = np.asarray(pose.sensor_pose_from_c2w(c2w).T_world_sensors[0], np.float32)
    view = dict(model=model, W=W, H=H, tq=tq, distorted=bool(distorted), focal_length=np.array([fx, fx * 1.03], np.float32),
                principal_point=np.array([W / 2 + 0.31, H / 2 - 0.23], np.float32), radial=np.zeros(6, np.float32),
                tangential=np.zeros(2, np.float32), thin_prism=np.zeros(4, np.float32), max_angle=0.0)
    if model == "pinhole" and distorted:
        view.update(radial=np.asarray(DISTORTION["radial"], np.float32), tangential=np.asarray(DISTORTION["tangential"], np.float32),
                    thin_prism=np.asarray(DISTORTION["thin_prism"], np.float32))
    if model == "fisheye":
        view["radial"] = np.asarray(FISHEYE_RADIAL + [0.0, 0.0], np.float32)
        view["max_angle"] = float(np.float32(cams.fisheye_max_angle(W, H, fx, fx * 1.03, W / 2 + 0.31, H / 2 - 0.23)))
    return view


def _sphere_hit(o, d, radius):
    """The far-side-excluded ray-sphere distance [n] (inf without a hit in front of the origin), o [n,3] or [3], d [n,3] unit."""
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - radius * radius
    disc = b * b - c
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.where(disc >= 0, disc, np.nan))
    near, far = -b - root, -b + root
    t = np.where(near > 0, near, far)
    return np.where(np.isfinite(t) & (t > 0), t, np.inf)


def _eye(azimuth_deg, elevation_deg):
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    return (CAMERA_DISTANCE * math.cos(el) * math.sin(az), -CAMERA_DISTANCE * math.sin(el), -CAMERA_DISTANCE * math.cos(el) * math.cos(az))


@functools.lru_cache(maxsize=None)
def sphere_views():
    """The ten views with their float32 planes: distance [H,W], rgba [H,W,4] (a smooth function of the hit point, some of it outside
    [0, 1] so that the clamp works), and for two of them a ray-origin plane (rays that start a little off the sensor position)."""
    specs = [("pinhole", 48, 40, _eye(17.3, 31.1), False), ("pinhole", 64, 64, _eye(108.7, 28.9), False),
             ("pinhole", 56, 48, _eye(196.9, 33.3), False), ("pinhole", 64, 60, _eye(287.1, 29.2), True),
             ("pinhole", 64, 56, _eye(62.4, -27.7), False), ("pinhole", 32, 32, _eye(151.2, -32.6), False),
             ("fisheye", 64, 64, _eye(243.9, -30.1), False), ("pinhole", 64, 48, _eye(331.3, -28.4), False),
             ("pinhole", 64, 64, _eye(11.3, 83.9), False), ("pinhole", 60, 64, _eye(101.7, -85.2), False)]
    views = []
    for n, (model, W, H, eye, distorted) in enumerate(specs):
        view = make_camera(model, W, H, eye, FOCAL * W, distorted)
        R, t = quat_rows(view["tq"], np.float64)
        d = pixel_rays(view).reshape(-1, 3)
        if n in (2, 6):      # rays that do not start at the sensor position
            rng = np.random.default_rng(190 + n)
            o = (0.02 * rng.standard_normal((1, 3)) + 0.004 * rng.standard_normal(d.shape)).astype(np.float32)
            view["ray_origin"] = o.reshape(H, W, 3)
        else:
            o = np.zeros_like(d, dtype=np.float32)
            view["ray_origin"] = None
        o64 = o.astype(np.float64)
        centre = t                                   # the world origin in the sensor frame
        rel = o64 - centre
        dist = np.minimum(_sphere_hit(rel, d, 1.0), _sphere_hit(rel, d, ENCLOSING_RADIUS))
        assert np.isfinite(dist).all()
        hit = rel + dist[:, None] * d                 # relative to the spheres' centre, sensor axes
        world = hit @ R                               # R^T applied: world axes
        rgb = 0.5 + 0.6 * np.stack([world[:, 0], world[:, 1], world[:, 2]], -1) / np.maximum(np.linalg.norm(world, axis=1, keepdims=True), 1e-9)
        view["distance"] = dist.astype(np.float32).reshape(H, W)
        view["rgba"] = np.concatenate([rgb, np.ones((len(rgb), 1))], 1).astype(np.float32).reshape(H, W, 4)
        views.append(view)
    return tuple(views)


@functools.lru_cache(maxsize=None)
def sphere_case(size, dims=None):
    """The sphere on a size^3 grid (or `dims`, voxel from `size`): dict(origin, voxel, dims, truncation, views)."""
    voxel = float(np.float32(2.0 * HALF_BOX / size))
    dims = (size, size, size) if dims is None else tuple(dims)
    origin = tuple(float(np.float32(-0.5 * voxel * n + o)) for n, o in zip(dims, ORIGIN_OFFSET))
    return dict(origin=origin, voxel=voxel, dims=dims, truncation=float(np.float32(TRUNCATION_VOXELS * voxel)), views=sphere_views())


# ---- the integration ----
def integrate_views(grid, views, dtype=np.float64, colours=True, origins=True):
    """The integration of `views` into an empty grid in `dtype`: dict(acc int64 [Z,Y,X], cnt, rgb_sum [Z,Y,X,3], rgb_cnt, near bool,
    near_views int (the views that made the voxel near), near_colour bool, updated bool)."""
    T = dtype
    X, Y, Z = grid["dims"]
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    origin, voxel, trunc = np.asarray(grid["origin"], np.float32).astype(T), T(np.float32(grid["voxel"])), T(np.float32(grid["truncation"]))
    p = np.stack([origin[0] + voxel * (i.ravel().astype(T) + T(0.5)), origin[1] + voxel * (j.ravel().astype(T) + T(0.5)),
                  origin[2] + voxel * (k.ravel().astype(T) + T(0.5))], -1)
    n = p.shape[0]
    acc, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rgb_sum, rgb_cnt = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    near_views, near_colour = np.zeros(n, np.int64), np.zeros(n, bool)
    for view in views:
        R, t = quat_rows(view["tq"], T)
        c = np.stack([R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1] + R[r, 2] * p[:, 2] + t[r] for r in range(3)], -1)
        u, v, valid, ok, margin, depth_margin = project(view, c, T)
        W, H = view["W"], view["H"]
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        with np.errstate(invalid="ignore"):
            edge = np.minimum(np.abs(u64 - np.rint(u64)), np.abs(v64 - np.rint(v64))) <= NEAR_PIXEL
            reach = ok & (u64 > -1) & (v64 > -1) & (u64 < W + 1) & (v64 < H + 1)      # in or beside the image
        near = (reach & edge) | (margin <= NEAR_REL) | (depth_margin <= NEAR_REL * float(trunc))
        px = np.clip(np.floor(np.where(valid, u64, 0)).astype(np.int64), 0, W - 1)
        py = np.clip(np.floor(np.where(valid, v64, 0)).astype(np.int64), 0, H - 1)
        D = np.asarray(view["distance"], np.float32)[py, px].astype(T)
        live = valid & (D != 0) & np.isfinite(D)
        o = np.zeros((n, 3), T)
        if origins and view.get("ray_origin") is not None:
            o = np.asarray(view["ray_origin"], np.float32)[py, px].astype(T)
        dx, dy, dz = c[:, 0] - o[:, 0], c[:, 1] - o[:, 1], c[:, 2] - o[:, 2]
        with np.errstate(invalid="ignore"):
            s = D - np.sqrt(dx * dx + dy * dy + dz * dz)
            s64 = s.astype(np.float64)
            near |= live & (np.abs(s64 + float(trunc)) <= NEAR_REL * float(trunc))
            near_colour |= live & (np.abs(s64 - float(trunc)) <= NEAR_REL * float(trunc))
            upd = live & (s >= -trunc)
            f = np.minimum(T(1), s / trunc)
            q = np.rint(np.where(upd, f * T(65536), 0)).astype(np.int64)
        acc += q
        cnt += upd
        if colours and view.get("rgba") is not None:
            with np.errstate(invalid="ignore"):
                col = upd & (np.abs(s) <= trunc)
            rgb = np.clip(np.nan_to_num(np.asarray(view["rgba"], np.float32)[py, px, :3].astype(T)), T(0), T(1))
            rgb_sum += np.where(col[:, None], np.rint(T(255) * rgb), 0).astype(np.int64)
            rgb_cnt += col
        near_views += near
    shape = (Z, Y, X)
    return dict(acc=acc.reshape(shape), cnt=cnt.reshape(shape), rgb_sum=rgb_sum.reshape(shape + (3,)), rgb_cnt=rgb_cnt.reshape(shape),
                near=(near_views > 0).reshape(shape), near_views=near_views.reshape(shape), near_colour=near_colour.reshape(shape),
                updated=(cnt > 0).reshape(shape))


@functools.lru_cache(maxsize=None)
def sphere_reference(size, dims=None, float32=False, colours=True, origins=True):
    case = sphere_case(size, dims)
    out = integrate_views(case, case["views"], np.float32 if float32 else np.float64, colours=colours, origins=origins)
    for a in out.values():
        a.setflags(write=False)
    return out


def float32_band(size, dims=None):
    """(largest |acc32 - acc64| over calm voxels, voxels whose cnt differs among the calm ones, calm voxels)."""
    r64, r32 = sphere_reference(size, dims), sphere_reference(size, dims, float32=True)
    calm = ~r64["near"] & (r64["updated"] | r32["updated"])
    return int(np.abs(r32["acc"] - r64["acc"])[calm].max()), int((r32["cnt"] != r64["cnt"])[calm].sum()), int(calm.sum())


# ---- the extraction, on the integer grid ----
CORNERS = tuple((c & 1, (c >> 1) & 1, c >> 2) for c in range(8))            # (dx, dy, dz) of corner dx + 2 dy + 4 dz
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))     # gut_hip.h's order


def extract(acc, cnt, rgb_sum, rgb_cnt, origin, voxel, min_count=1):
    """(vertices float64 [V,3], colours float64 [V,3], faces int64 [F,3]) of gut_hip.h's surface nets on the integer state [Z,Y,X]."""
    acc, cnt = np.asarray(acc, np.int64), np.asarray(cnt, np.int64)
    Z, Y, X = acc.shape
    observed, inside = cnt >= min_count, acc < 0
    with np.errstate(all="ignore"):
        f = np.asarray(np.float32(acc), np.float64) / (np.asarray(np.float32(cnt), np.float64) * 65536.0)
    if min(X, Y, Z) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    corner = lambda a, c: a[c[2]:Z - 1 + c[2], c[1]:Y - 1 + c[1], c[0]:X - 1 + c[0]]
    full = np.logical_and.reduce([corner(observed, c) for c in CORNERS])
    n_in = sum(corner(inside, c).astype(np.int64) for c in CORNERS)
    active = full & (n_in > 0) & (n_in < 8)
    total, crossings = np.zeros(active.shape + (3,)), np.zeros(active.shape, np.int64)
    for c0, c1 in EDGES:
        axis = int(np.log2(c1 - c0))
        f0, f1 = corner(f, CORNERS[c0]), corner(f, CORNERS[c1])
        cross = active & (corner(inside, CORNERS[c0]) != corner(inside, CORNERS[c1]))
        with np.errstate(all="ignore"):
            t = np.where(cross, f0 / (f0 - f1), 0.0)
        at = np.zeros(active.shape + (3,))
        at[...] = CORNERS[c0]
        at[..., axis] = t
        total += np.where(cross[..., None], at, 0.0)
        crossings += cross
    kk, jj, ii = np.nonzero(active)            # C order of [Z-1,Y-1,X-1]: ascending cell linear index
    mean = total[kk, jj, ii] / crossings[kk, jj, ii][:, None]
    vertices = np.asarray(origin, np.float64) + float(voxel) * (np.stack([ii, jj, kk], -1) + 0.5 + mean)
    colours = np.full((len(kk), 3), 0.5)
    if rgb_sum is not None:
        rgb_sum, rgb_cnt = np.asarray(rgb_sum, np.int64), np.asarray(rgb_cnt, np.int64)
        with np.errstate(all="ignore"):
            per = rgb_sum / (255.0 * rgb_cnt[..., None])
        have = rgb_cnt > 0
        s = sum(np.where(corner(have, c)[..., None], corner(per, c), 0.0) for c in CORNERS)
        m = sum(corner(have, c).astype(np.int64) for c in CORNERS)
        with np.errstate(all="ignore"):
            colours = np.where(m[kk, jj, ii][:, None] > 0, s[kk, jj, ii] / m[kk, jj, ii][:, None], 0.5)
    vertex_of = np.full((Z, Y, X), -1, np.int64)        # by the cell's lower corner
    vertex_of[kk, jj, ii] = np.arange(len(kk))
    cell_full = np.zeros((Z, Y, X), bool)
    cell_full[:Z - 1, :Y - 1, :X - 1] = full
    step = ((0, 0, 1), (0, 1, 0), (1, 0, 0))             # e_x, e_y, e_z as (dk, dj, di)
    quads = []
    pk, pj, pi = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    linear = (pk * Y + pj) * X + pi
    for axis in range(3):
        ea, eb, ec = (np.array(step[(axis + n) % 3]) for n in range(3))
        ok = np.ones((Z, Y, X), bool)
        cells = []
        for off in (-eb - ec, -ec, 0 * ea, -eb):
            qk, qj, qi = pk + off[0], pj + off[1], pi + off[2]
            inb = (qk >= 0) & (qj >= 0) & (qi >= 0)
            ok &= inb & cell_full[np.maximum(qk, 0), np.maximum(qj, 0), np.maximum(qi, 0)]
            cells.append((qk, qj, qi))
        ek, ej, ei = pk + ea[0], pj + ea[1], pi + ea[2]
        inb = (ek < Z) & (ej < Y) & (ei < X)
        other = inside[np.minimum(ek, Z - 1), np.minimum(ej, Y - 1), np.minimum(ei, X - 1)]
        ok &= inb & (inside != other)
        sel = np.nonzero(ok)
        v = [vertex_of[c[0][sel], c[1][sel], c[2][sel]] for c in cells]
        p_in = inside[sel]
        q = np.stack([v[0], np.where(p_in, v[1], v[3]), v[2], np.where(p_in, v[3], v[1])], -1)
        quads.append((linear[sel] * 3 + axis, q))
    keys = np.concatenate([k for k, _ in quads])
    quad = np.concatenate([q for _, q in quads])[np.argsort(keys, kind="stable")]
    assert (quad >= 0).all()
    faces = np.stack([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return vertices, colours, faces


@functools.lru_cache(maxsize=None)
def sphere_mesh(size):
    case, ref = sphere_case(size), sphere_reference(size)
    out = extract(ref["acc"], ref["cnt"], ref["rgb_sum"], ref["rgb_cnt"], case["origin"], case["voxel"])
    for a in out:
        a.setflags(write=False)
    return out


def mesh_report(vertices, faces, voxel, centre=(0.0, 0.0, 0.0), radius=1.0):
    """What the sphere tests assert, of any mesh: dict(V, F, E, boundary_edges (in exactly one triangle), crowded_edges (in more than
    two), unbalanced_edges (a directed edge without as many reverses), inward (triangles whose normal does not point away from the
    centre), euler (V - E + F), worst (largest | |v - centre| - radius | in voxel edges))."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = lambda a, b: a * (len(v) + 1) + b
    fwd, fwd_n = np.unique(key(directed[:, 0], directed[:, 1]), return_counts=True)
    back = dict(zip(*np.unique(key(directed[:, 1], directed[:, 0]), return_counts=True)))
    unbalanced = sum(1 for k, n in zip(fwd.tolist(), fwd_n.tolist()) if back.get(k, 0) != n)
    und, und_n = np.unique(key(directed.min(1), directed.max(1)), return_counts=True)
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    out = ((v[f].mean(1) - np.asarray(centre)) * normal).sum(1)
    return dict(V=len(v), F=len(f), E=len(und), boundary_edges=int((und_n == 1).sum()), crowded_edges=int((und_n > 2).sum()),
                unbalanced_edges=int(unbalanced), inward=int((out <= 0).sum()), euler=len(v) - len(und) + len(f),
                worst=float(np.abs(np.linalg.norm(v - np.asarray(centre), axis=1) - radius).max() / voxel) if len(v) else 0.0)


def check_closed_sphere(report, label):
    """The assertions of the sphere, on a mesh_report."""
    print(f"[mesh {label}] {report}")
    assert report["V"] > 0 and report["F"] > 0
    assert report["boundary_edges"] == 0, f"{label}: {report['boundary_edges']} edges lie in exactly one triangle"
    assert report["unbalanced_edges"] == 0, f"{label}: {report['unbalanced_edges']} directed edges without as many reverses"
    assert report["inward"] == 0, f"{label}: {report['inward']} triangles face the centre"
    if report["crowded_edges"] == 0:
        assert report["euler"] == 2, f"{label}: V - E + F = {report['euler']}"
    assert report["worst"] <= 1.0, f"{label}: a vertex lies {report['worst']:.3f} voxel edges off the sphere"


assert K_BAND == 2.5
