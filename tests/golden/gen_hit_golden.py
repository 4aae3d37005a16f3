"""Writes tests/golden/hit_golden.npz: inputs, and what the reference's OWN per-hit header returns for them.

Needs oracle/_ref/libgut_refhits.so (`make -C oracle _ref`, or __graft_entry__.build(), with the reference tree beside the
repository): the reference's kernels/cuda/models/gaussianParticles.cuh compiled for the host behind oracle/ref_host/shim.h.
Every expected value in the file was returned by that library; the oracle only supplies what the reference cannot give here
(tile lists, forward finals and world rays of scene (c): its projection and forward are Slang / tiny-cuda-nn).  The file holds
arrays only.  Three parts (tests/reference_hit_cases.py names the classes; tests/test_cpu_reference_hits.py reads the file):

  (a) hit_*  per degree 256 seeded per-hit cases of processHitBwd<n, false, false>: ray, particle, running state, finals,
      cotangents -> accept decision, state after, density gradient [11], feature gradient [3]; response / response gradient.
  (b) sh_*   per SH degree 0..3, 128 directions x coefficient rows: radianceFromSpH clamped / unclamped, and the five-argument
      radianceFromSpHBwd for a drawn cotangent; quat_* quaternionWXYZToMatrix.
  (c) scene_* one 48 x 40 view of 12 Gaussians per degree: each ray walks its tile's list in the oracle's order through the
      reference's per-hit backward exactly as the unsorted backward's loop does (gutKBufferRenderer.cuh:336-384: an invalid id
      ends the ray :343-346, an alive ray calls processHitBwd :356-373 and ends once its transmittance is below the threshold
      :374-376; the features it passes are max(precomputed, 0) :324; the depth arguments arrive mis-ordered,
      shRadiativeGaussianParticles.cuh:404-406 — SURVEY §8a quirk 1 — so the integrated depth is the ray's untouched 0 and the
      running depth a copy of the forward's distance); the fp32 per-hit gradients are summed per Gaussian in float64, the summed
      feature gradients go through the reference's radianceFromSpHBwd along the oracle's view direction.
"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import reference_hit_cases as rc          # noqa: E402
from tests.common import cams, make_view             # noqa: E402

oracle = importlib.import_module("oracle.oracle")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _short_mantissa(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)


def _rows64(q):
    return rc._rows64(q)


def draw_hit_cases(degree, rng):
    """256 cases: [0,168) generic, then 16 clamped alpha, 16 terminating, 8 + 8 residual clamps, 8 through the centre,
    8 + 8 rejected (response, alpha), 16 needles.  The ray is placed in the particle's canonical space (unit direction u, closest
    approach c perpendicular to it with |c| = r, origin c - t u) and mapped back, so r sets the response."""
    n = rc.CASES_PER_DEGREE
    kind = np.concatenate([np.full(168, 0), np.full(16, 1), np.full(16, 2), np.full(8, 3), np.full(8, 4), np.full(8, 5), np.full(8, 6),
                           np.full(8, 7), np.full(16, 8)])
    assert kind.size == n
    pos = rng.normal(scale=0.5, size=(n, 3))
    scale = np.exp(rng.uniform(-1.5, 0.0, size=(n, 3)))
    needle = kind == 8
    long_axis = rng.integers(0, 3, size=n)
    scale[needle] = np.exp(rng.uniform(-1.0, 0.0, size=(16, 1))) * np.where(np.arange(3)[None, :] == long_axis[needle, None], 1.0, 0.05)
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat = quat.astype(np.float32).astype(np.float64)
    scale = scale.astype(np.float32).astype(np.float64)
    dens = rng.uniform(0.05, 0.95, size=n)
    r = rng.uniform(0.0, 2.9, size=n)
    r[kind == 1] = rng.uniform(0.0, 0.004, size=16); dens[kind == 1] = 1.0                      # gres * density >= 0.99
    r[kind == 2] = rng.uniform(0.0, 0.2, size=16); dens[kind == 2] = rng.uniform(0.8, 0.95, size=16)
    r[(kind == 3) | (kind == 4)] = rng.uniform(0.0, 1.5, size=16)
    r[kind == 6] = rng.uniform(3.05, 4.0, size=8)                                               # response below 0.0113
    r[kind == 7] = rng.uniform(0.0, 1.5, size=8); dens[kind == 7] = rng.uniform(0.001, 0.003, size=8)   # alpha below 1/255
    r[kind == 8] = rng.uniform(0.0, 2.5, size=16)
    u = _unit(rng, n)
    c = np.cross(u, _unit(rng, n)); c = c / np.linalg.norm(c, axis=1, keepdims=True) * r[:, None]
    t = rng.uniform(1.0, 5.0, size=n)
    gro = c - t[:, None] * u
    rows = _rows64(quat)
    ray_d = np.einsum("nji,nj->ni", rows, scale * u); ray_d /= np.linalg.norm(ray_d, axis=1, keepdims=True)
    ray_o = pos + np.einsum("nji,nj->ni", rows, scale * gro)
    particle = np.zeros((n, 12), np.float32)
    particle[:, 0:3] = pos; particle[:, 3] = dens; particle[:, 4:8] = quat; particle[:, 8:11] = scale
    if needle.any():   # exactly 20:1 in fp32: the two short axes are the long one times 0.05, rounded once
        s = particle[needle, 8:11]
        long_ = s.max(1, keepdims=True)
        particle[needle, 8:11] = np.where(s == long_, long_, np.float32(0.05) * long_)
    ray_o = ray_o.astype(np.float32); ray_d = ray_d.astype(np.float32)
    ray_o[kind == 5] = particle[kind == 5, 0:3]                                                 # the ray starts AT the centre: gsqdist == 0
    feat = np.maximum(rng.uniform(-0.2, 1.0, size=(n, 3)), 0.0).astype(np.float32)
    # running state before the hit, finals behind it, cotangents
    T = rng.uniform(0.05, 1.0, size=n)
    T[kind == 2] = rng.uniform(1.0e-4, 3.0e-4, size=16)                                         # (1 - alpha) T <= 1e-4
    rad = rng.uniform(0.0, 0.5, size=(n, 3)); depth = rng.uniform(0.0, 2.0, size=n)
    T_fin = T * rng.uniform(0.0, 0.9, size=n)
    rad_fin = rad + T[:, None] * rng.uniform(0.3, 1.5, size=(n, 3))
    depth_fin = depth + T * rng.uniform(4.0, 9.0, size=n)
    depth_fin[kind == 3] = depth[kind == 3] * rng.uniform(0.0, 1.0, size=8)                     # integratedDepth - depth < 0
    sel = np.nonzero(kind == 4)[0]
    rad_fin[sel, rng.integers(0, 3, size=sel.size)] = rad[sel, 0] * 0.0 - 0.01                 # one residual colour component negative
    state = np.concatenate([T[:, None], rad, depth[:, None]], 1).astype(np.float32)
    finals = np.concatenate([T_fin[:, None], rad_fin, depth_fin[:, None]], 1).astype(np.float32)
    cot = rng.normal(size=(n, 5)).astype(np.float32)
    # the non-geometric inputs keep 12 mantissa bits (the file compresses; every product and sum they enter has a full-width partner)
    feat, state, finals, cot = (_short_mantissa(v) for v in (feat, state, finals, cot))
    return dict(ray_ori=ray_o, ray_dir=ray_d, particle=particle, feat=feat, state=state, finals=finals, cot=cot)


def run_hit_cases(units, degree, case):
    n = case["ray_ori"].shape[0]
    out = dict(accepted=np.zeros(n, np.int32), state_after=np.zeros((n, 5), np.float32), density_grad=np.zeros((n, 11), np.float32),
               feat_grad=np.zeros((n, 3), np.float32))
    for i in range(n):
        a, st, g11, g3 = units.hit_bwd(degree, case["ray_ori"][i], case["ray_dir"][i], case["particle"][i], case["feat"][i], rc.THRESHOLDS,
                                       case["finals"][i], case["cot"][i], case["state"][i])
        out["accepted"][i] = a; out["state_after"][i] = st; out["density_grad"][i] = g11; out["feat_grad"][i] = g3
    return out


def response_inputs(rng):
    """squared canonical distances: 0, tiny, a sweep through every kernel's support, and beyond it"""
    d2 = np.concatenate([[0.0, 1e-12, 1e-6, 8.9, 9.0, 9.1, 9.2033, 16.0, 40.0], rng.uniform(0.0, 12.0, size=119)]).astype(np.float32)
    return d2, rng.normal(size=d2.size).astype(np.float32)


def draw_sh_cases(rng):
    n = rc.SH_CASES
    d = _unit(rng, n).astype(np.float32)
    d[:3] = np.eye(3, dtype=np.float32)
    sph = rng.normal(scale=0.5, size=(n, 16, 3))
    sph[:, 0, :] = rng.normal(loc=-0.5, scale=2.0, size=(n, 3))    # a DC term that often leaves a channel negative: the clamp and the mask act
    return d, sph.reshape(n, 48).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


def scene_c():
    """12 Gaussians in front of a camera at (0, 0, -4) looking along +z: [0] covers every tile, [1, 2] overlap, [3..7] five near-opaque
    ones stacked along one line of sight in front (rays through their middle terminate), [8] density 1 on the optical axis, [9] a
    20:1 needle, [10, 11] scattered."""
    rng = np.random.default_rng(20260)
    sight = np.array([1.1, -0.6, 3.0])
    stack = [np.array(rc.SCENE_EYE) + t * sight for t in (1.0, 1.03, 1.06, 1.09, 1.12)]
    pos = np.array([[0.0, 0.0, 1.0], [-1.0, 0.3, 0.0], [-0.85, 0.38, 0.15], *stack,
                    [0.0, 0.0, -0.5], [0.2, 0.9, 0.2], [-1.3, -1.0, 0.4], [0.9, 0.8, -0.3]])
    scale = np.array([[2.5, 2.2, 0.6], [0.45, 0.35, 0.3], [0.4, 0.5, 0.3], [0.9, 0.9, 0.1], [0.9, 0.8, 0.1], [0.8, 0.9, 0.1], [0.9, 0.9, 0.1], [0.85, 0.9, 0.1],
                      [0.25, 0.25, 0.25], [0.8, 0.04, 0.04], [0.3, 0.5, 0.4], [0.3, 0.2, 0.4]])
    dens = np.array([0.6, 0.7, 0.5, 0.97, 0.96, 0.98, 0.95, 0.975, 1.0, 0.8, 0.4, 0.9])    # (a stack clamped at 0.99 would end rays at T = 0.01^2, ON the threshold)
    quat = rng.normal(size=(12, 4)); quat[3:9] = (1, 0, 0, 0); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    d12 = np.zeros((12, 12), np.float32)
    d12[:, 0:3] = pos; d12[:, 3] = dens; d12[:, 4:8] = quat; d12[:, 8:11] = scale
    sph = rng.normal(scale=0.3, size=(12, 16, 3)); sph[:, 0, :] = rng.uniform(-1.0, 2.5, size=(12, 3))
    rgba_grad = rng.normal(size=(rc.SCENE_H, rc.SCENE_W, 4)).astype(np.float32)
    dist_grad = (0.2 * rng.normal(size=(rc.SCENE_H, rc.SCENE_W, 1))).astype(np.float32)
    return d12, sph.reshape(12, 48).astype(np.float32), rgba_grad, dist_grad


def scene_view():
    return make_view("pinhole", rc.SCENE_W, rc.SCENE_H, cams.look_at_c2w(rc.SCENE_EYE, rc.SCENE_TARGET), fx=rc.SCENE_FX)


def walk_scene(units, degree, d12, sph, rgba_grad, dist_grad):
    """The unsorted backward's per-ray loop (module docstring) over the oracle's tile lists, the per-hit step the reference's."""
    view = scene_view()
    W, H = rc.SCENE_W, rc.SCENE_H
    prm = oracle.default_params(); prm.kernel_degree = degree
    assert oracle.lib().oracle_get_variant() == 0
    fwd = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=rc.SCENE_SH_DEGREE, params=prm)
    wo, wd, alive = oracle.world_rays(view["oracle_cam"], view["ro"], view["rd"])
    gx = (W + 15) // 16
    g12 = np.zeros((12, 12), np.float64); gf = np.zeros((12, 3), np.float64)
    pairs = terminated = 0
    feat = np.maximum(fwd["feat"], np.float32(0.0))
    for py in range(H):
        for px in range(W):
            pix = py * W + px
            if not alive[pix]:
                continue
            beg, end = (int(v) for v in fwd["tile_ranges"][(py // 16) * gx + px // 16])
            rgba, rg = fwd["rgba"][py, px], rgba_grad[py, px]
            finals = np.array([np.float32(1.0) - rgba[3], rgba[0], rgba[1], rgba[2], 0.0], np.float32)      # rayPayloadBackward.cuh:49-53; quirk 1
            cot = np.array([np.float32(-1.0) * rg[3], rg[0], rg[1], rg[2], dist_grad[py, px, 0]], np.float32)
            state = np.array([1.0, 0.0, 0.0, 0.0, 0.0], np.float32)
            for k in range(beg, end):
                pid = int(fwd["sorted_ids"][k])
                if pid == 0xFFFFFFFF:
                    break
                state[4] = fwd["dist"][py, px, 0]          # quirk 1: a by-value copy of the forward's distance, every call
                acc, state, g11, g3 = units.hit_bwd(degree, wo[pix], wd[pix], d12[pid], feat[pid], rc.THRESHOLDS, finals, cot, state)
                if acc:
                    pairs += 1
                    g12[pid, :11] += g11.astype(np.float64); gf[pid] += g3.astype(np.float64)
                if state[0] < rc.THRESHOLDS[2]:
                    terminated += 1
                    break
    g48 = np.zeros((12, 48), np.float64)
    for i in range(12):
        if fwd["tiles_count"][i]:
            g48[i] = units.sh_radiance_bwd(rc.SCENE_SH_DEGREE, oracle.view_direction(view["oracle_cam"], d12[i, 0:3]), gf[i].astype(np.float32), fwd["feat"][i])
    return dict(g12=g12, g48=g48, pairs=pairs, terminated=terminated, fwd=fwd)


def check_scene(degree, d12, res):
    fwd = res["fwd"]
    T = (rc.SCENE_W + 15) // 16 * ((rc.SCENE_H + 15) // 16)
    assert T == 9 and fwd["tiles_count"][0] == T, "Gaussian 0 must cover every tile"
    assert float(fwd["hits"].max()) >= 3, "rays through the overlapping pair take several hits"
    assert res["terminated"] >= 3, "some rays terminate behind the near-opaque stack"
    assert d12[8, 3] == 1.0 and d12[8, 0] == 0 and d12[8, 1] == 0
    assert np.abs(res["g12"][:, :11]).max(1).min() > 0, "every Gaussian receives a gradient"


def main():
    units = oracle.HitUnits.reference()
    assert units is not None, f"{oracle.REF_HITS_SO} is missing: make -C oracle _ref"
    out = dict(degrees=np.array(rc.DEGREES, np.int32), thresholds=rc.THRESHOLDS)
    rng = np.random.default_rng(480738)
    d2, rgrad = response_inputs(rng)
    out["resp_d2"], out["resp_cot"] = d2, rgrad
    for n in rc.DEGREES:
        case = draw_hit_cases(n, rng)
        res = run_hit_cases(units, n, case)
        pop = rc.check_populations(n, rc.hit_classes(n, case["ray_ori"], case["ray_dir"], case["particle"], case["feat"], case["finals"],
                                                     case["state"], res["accepted"]))
        print(f"degree {n}: {pop}")
        for k, v in {**case, **res}.items():
            out[f"hit{n}_{k}"] = v
        resp = np.array([units.response(n, v) for v in d2], np.float32)
        out[f"resp{n}"] = resp
        out[f"resp{n}_grad"] = np.array([units.response_grad(n, a, b, c) for a, b, c in zip(d2, resp, rgrad)], np.float32)
    sh_dir, sh_rows, sh_cot = draw_sh_cases(rng)
    out["sh_dir"], out["sh_rows"], out["sh_cot"] = sh_dir, sh_rows, sh_cot
    for deg in range(4):
        cl = np.stack([units.sh_radiance(deg, r, d, True) for r, d in zip(sh_rows, sh_dir)])
        un = np.stack([units.sh_radiance(deg, r, d, False) for r, d in zip(sh_rows, sh_dir)])
        assert int((un <= 0).any(1).sum()) >= rc.MIN_CLASS and int((un > 0).all(1).sum()) >= rc.MIN_CLASS
        out[f"sh{deg}_clamped"], out[f"sh{deg}_unclamped"] = cl, un
        out[f"sh{deg}_grad"] = np.stack([units.sh_radiance_bwd(deg, d, g, u) for d, g, u in zip(sh_dir, sh_cot, un)])
    q = rng.normal(size=(32, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = q.astype(np.float32); q[0] = (1, 0, 0, 0)
    out["quat"], out["quat_rows"] = q, np.stack([units.quat_rows(v) for v in q])
    d12, sph, rgba_grad, dist_grad = scene_c()
    out.update(scene_d12=d12, scene_sph=sph, scene_rgba_grad=rgba_grad, scene_dist_grad=dist_grad)
    for n in rc.DEGREES:
        res = walk_scene(units, n, d12, sph, rgba_grad, dist_grad)
        check_scene(n, d12, res)
        out[f"scene{n}_g12"], out[f"scene{n}_g48"], out[f"scene{n}_pairs"] = res["g12"], res["g48"], np.int64(res["pairs"])
        print(f"scene degree {n}: {res['pairs']} accepted pairs, {res['terminated']} rays terminated, M = {res['fwd']['M']}")
    path = rc.GOLDEN
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
