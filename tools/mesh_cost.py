"""Measures gut_tsdf_integrate and the surface nets at 256^3 and 512^3 with 1237 x 822 planes (analytic
sphere-in-sphere planes, eight pinhole views), against the same update in torch tensor ops, alternating in one process, and a 2 GiB
device copy.  One JSON line per figure on stdout; --out FILE keeps them too.

    python tools/mesh_cost.py [--out FILE]
"""
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mesh = importlib.import_module("3dgrut_amd.mesh")
_capi = importlib.import_module("3dgrut_amd._capi")
cams = importlib.import_module("3dgrut_amd.cameras")
pose = importlib.import_module("3dgrut_amd.pose")
DEV = "cuda:0"
W, H, FX = 1237, 822, 1000.0
OUT = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def quat_rt(tq):
    t = torch.tensor(tq[:3], dtype=torch.float32, device=DEV)
    x, y, z, w = (float(v) for v in tq[3:7])
    R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float32, device=DEV)
    return R, t


def make_views():
    views = []
    for n in range(8):
        az, el = math.radians(17.3 + 45.0 * n), math.radians(30.0 if n % 2 else -28.0)
        eye = (3.5 * math.cos(el) * math.sin(az), -3.5 * math.sin(el), -3.5 * math.cos(el) * math.cos(az))
        c2w = cams.look_at_c2w(eye, (0.0, 0.0, 0.0))
        tq = np.asarray(pose.sensor_pose_from_c2w(c2w).T_world_sensors[0], np.float32)
        R, t = quat_rt(tq)
        ys, xs = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float64) + 0.5, torch.arange(W, device=DEV, dtype=torch.float64) + 0.5, indexing="ij")
        d = torch.stack([(xs - W / 2) / FX, (ys - H / 2) / FX, torch.ones_like(xs)], -1)
        d = d / d.norm(dim=-1, keepdim=True)
        rel = -t.double()
        b = (rel * d).sum(-1)
        dist = torch.full_like(b, float("inf"))
        for radius in (6.0, 1.0):
            disc = b * b - ((rel * rel).sum() - radius * radius)
            root = torch.sqrt(disc.clamp_min(0))
            near = torch.where(-b - root > 0, -b - root, -b + root)
            dist = torch.where(disc >= 0, torch.minimum(dist, near), dist)
        cam = _capi.GutCamera()
        cam.model, cam.shutter = _capi.CAMERA_PINHOLE, _capi.SHUTTER_GLOBAL
        cam.principal_point[:] = [W / 2, H / 2]
        cam.focal_length[:] = [FX, FX]
        cam.pose_start[:] = [float(v) for v in tq]
        cam.pose_end[:] = [float(v) for v in tq]
        rgba = torch.rand((H, W, 4), device=DEV)
        views.append(dict(camera=cam, distance=dist.float().contiguous(), rgba=rgba, ray_origin=None, R=R, t=t))
    return views


def torch_integrate(p, acc, cnt, rgb_sum, rgb_cnt, trunc, view):
    """The same update in tensor ops, one view (undistorted pinhole, rays from the sensor position)."""
    c = p @ view["R"].T + view["t"]
    rz = 1.0 / c[:, 2]
    u, v = c[:, 0] * rz * FX + W / 2, c[:, 1] * rz * FX + H / 2
    valid = (c[:, 2] > 0) & (u > 0) & (v > 0) & (u < W) & (v < H)
    px, py = u.floor().clamp(0, W - 1).long(), v.floor().clamp(0, H - 1).long()
    pixel = py * W + px
    D = view["distance"].reshape(-1)[pixel]
    s = D - c.norm(dim=1)
    upd = valid & (D != 0) & torch.isfinite(D) & (s >= -trunc)
    acc += torch.where(upd, torch.round(torch.clamp(s / trunc, max=1.0) * 65536.0), torch.zeros_like(s)).to(torch.int32)
    cnt += upd.to(torch.int32)
    col = upd & (s.abs() <= trunc)
    rgb = view["rgba"].reshape(-1, 4)[pixel, :3].clamp(0, 1)
    rgb_sum += torch.where(col[:, None], torch.round(255.0 * rgb), torch.zeros_like(rgb)).to(torch.int32)
    rgb_cnt += col.to(torch.int32)


def timed(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(t, 3) for t in times]


def main():
    torch.cuda.init()
    views = make_views()
    src = torch.empty(1 << 29, dtype=torch.float32, device=DEV)      # 2 GiB
    dst = torch.empty_like(src)
    ms, _ = timed(lambda: dst.copy_(src), 5)
    copy_rate = 2 * src.numel() * 4 / (ms * 1e-3)
    say(what="device copy 2 GiB", ms=ms, bytes_per_s=copy_rate)
    del src, dst
    for size in (256, 512):
        voxel = 2.6 / size
        make = lambda: mesh.TSDFVolume((-1.3 + 0.0137, -1.3 - 0.0071, -1.3 + 0.0213), voxel, (size,) * 3, 4 * voxel, device=DEV)
        # the byte count of a launch from its inputs: the voxels its views update, on an empty volume
        probe = make().integrate(views[:1])
        upd1, col1 = int((probe.cnt > 0).sum()), int((probe.rgb_cnt > 0).sum())
        probe = make().integrate(views)
        upd8, col8 = int((probe.cnt > 0).sum()), int((probe.rgb_cnt > 0).sum())
        del probe
        vol = make()
        reps = 5 if size == 256 else 3
        vol.integrate(views[:1])            # warm-up
        torch.cuda.synchronize()
        k1, k1_all = timed(lambda: vol.integrate(views[:1]), reps)
        k8, k8_all = timed(lambda: vol.integrate(views), reps)
        # torch on the same state
        kk, jj, ii = torch.meshgrid(*(torch.arange(size, device=DEV, dtype=torch.float32) for _ in range(3)), indexing="ij")
        p = torch.stack([vol.origin[0] + voxel * (ii.reshape(-1) + 0.5), vol.origin[1] + voxel * (jj.reshape(-1) + 0.5),
                         vol.origin[2] + voxel * (kk.reshape(-1) + 0.5)], -1)
        del kk, jj, ii
        tv = mesh.TSDFVolume(vol.origin, voxel, vol.dims, 4 * voxel, device=DEV)
        flat = (tv.acc.view(-1), tv.cnt.view(-1), tv.rgb_sum.view(-1, 3), tv.rgb_cnt.view(-1))
        torch_integrate(p, *flat, tv.truncation, views[0])      # warm-up
        torch.cuda.synchronize()
        rounds = []
        for _ in range(reps):               # alternating
            t1, _ = timed(lambda: torch_integrate(p, *flat, tv.truncation, views[0]), 1)
            a1, _ = timed(lambda: vol.integrate(views[:1]), 1)
            a8, _ = timed(lambda: vol.integrate(views), 1)
            rounds.append((t1, a1, a8))
        t1, a1, a8 = (float(np.median([r[i] for r in rounds])) for i in range(3))
        # agreement of the torch statement with the kernel on one view, for the record
        chk, ref = make().integrate(views[:1]), mesh.TSDFVolume(vol.origin, voxel, vol.dims, 4 * voxel, device=DEV)
        torch_integrate(p, ref.acc.view(-1), ref.cnt.view(-1), ref.rgb_sum.view(-1, 3), ref.rgb_cnt.view(-1), ref.truncation, views[0])
        differ = int((chk.cnt != ref.cnt).sum())
        del p, tv, flat, chk, ref
        say(what="integrate", size=size, voxels=size ** 3, kernel_1_view_ms=k1, kernel_8_views_ms=k8, kernel_8_views_ms_per_view=k8 / 8,
            alternating_torch_1_view_ms=t1, alternating_kernel_1_view_ms=a1, alternating_kernel_8_views_ms_per_view=a8 / 8,
            torch_over_kernel_1_view=t1 / a1, one_view_over_eight_view_per_view=a1 / (a8 / 8), all_1=k1_all, all_8=k8_all,
            updated_voxels_1=upd1, coloured_voxels_1=col1, updated_voxels_8=upd8, coloured_voxels_8=col8,
            state_bytes_1=16 * upd1 + 32 * col1, state_bytes_8=16 * upd8 + 32 * col8,
            bytes_per_s_1=(16 * upd1 + 32 * col1) / (k1 * 1e-3), bytes_per_s_8=(16 * upd8 + 32 * col8) / (k8 * 1e-3),
            share_of_copy_rate_1=(16 * upd1 + 32 * col1) / (k1 * 1e-3) / copy_rate, share_of_copy_rate_8=(16 * upd8 + 32 * col8) / (k8 * 1e-3) / copy_rate,
            voxels_where_torch_and_kernel_cnt_differ=differ)
        fresh = make().integrate(views)
        fresh.extract()                     # warm-up
        torch.cuda.synchronize()
        e, e_all = timed(lambda: fresh.extract(), 3)
        v, c, f = fresh.extract()
        say(what="extract", size=size, ms=e, all=e_all, vertices=int(v.shape[0]), faces=int(f.shape[0]))
        del fresh, vol, v, c, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
