"""What tests/golden/hit_golden.npz holds, and the classes its per-hit cases must populate.

The fixture records inputs and what the reference's OWN per-hit header returned for them (compiled for the host:
oracle/ref_host/, tests/golden/gen_hit_golden.py).  This module is shared by the generator, which asserts the population of every
class before it writes the file, and by tests/test_cpu_reference_hits.py, which re-asserts it from the file: the classes are
conditions on the INPUTS, evaluated here in float64 from the inputs alone (and the recorded accept decision).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hit_golden.npz")
DEGREES = (0, 1, 2, 3, 4, 5, 8)          # the seven kernels the reference instantiates (gaussianParticles.cuh:263-304)
CASES_PER_DEGREE = 256
SH_CASES = 128
THRESHOLDS = np.array([0.0113, 1.0 / 255.0, 1e-4], np.float32)   # min response, min alpha, min transmittance (render/3dgut.yaml)
MIN_ACCEPTED, MIN_CLASS = 0.6, 8

# scene (c): 48 x 40 = 3 x 3 tiles with a ragged last row and column
SCENE_W, SCENE_H, SCENE_FX, SCENE_EYE, SCENE_TARGET, SCENE_SH_DEGREE = 48, 40, 44.0, (0.0, 0.0, -4.0), (0.0, 0.0, 0.0), 3


def _response64(degree, d2):
    r = np.sqrt(d2)
    if degree == 0:
        return np.maximum(1.0 - 0.329630334487 * r, 0.0)
    return np.exp(-4.5 * (r / 3.0) ** degree)


def _rows64(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y),
                     2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x),
                     2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def hit_classes(degree, ray_ori, ray_dir, particle12, feat3, finals, state, accepted):
    """Boolean masks [n] per class of the issue's list, from float64 arithmetic on the inputs.  `accepted` is the recorded decision."""
    o, d, g = (np.asarray(v, np.float64) for v in (ray_ori, ray_dir, particle12))
    f, fin, st = (np.asarray(v, np.float64) for v in (feat3, finals, state))
    s, dens = g[:, 8:11], g[:, 3]
    rows = _rows64(g[:, 4:8])
    gro = np.einsum("nij,nj->ni", rows, o - g[:, 0:3]) / s
    grdu = np.einsum("nij,nj->ni", rows, d) / s
    ln = np.linalg.norm(grdu, axis=1, keepdims=True)
    grd = grdu / np.where(ln > 0, ln, 1.0)
    d2 = (np.cross(grd, gro) ** 2).sum(1)
    resp = _response64(degree, d2)
    alpha = np.minimum(0.99, resp * dens)
    acc = np.asarray(accepted).astype(bool)
    proj = -(grd * gro).sum(1)
    gdist = np.linalg.norm(s * grd * proj[:, None], axis=1)
    T, Tn = st[:, 0], (1 - alpha) * st[:, 0]
    depth_after = st[:, 4] + alpha * T * gdist
    rad_after = st[:, 1:4] + (alpha * T)[:, None] * f
    open_ = acc & (Tn > float(THRESHOLDS[2]))        # the residuals are taken, not replaced by zero
    smin, smax = s.min(1), s.max(1)
    return dict(
        accepted=acc,
        alpha_clamped=acc & (resp * dens >= 0.99),
        terminates=acc & (Tn <= float(THRESHOLDS[2])),
        residual_depth_negative=open_ & (fin[:, 4] - depth_after < 0),
        residual_colour_negative=open_ & ((fin[:, 1:4] - rad_after) < 0).any(1),
        through_centre=acc & (d2 == 0) & (gdist == 0),
        rejected_by_response=~acc & (resp < float(THRESHOLDS[0])),
        rejected_by_alpha=~acc & (resp > float(THRESHOLDS[0])) & (resp * dens < float(THRESHOLDS[1])),
        needle=(smax >= 19.99 * smin),
    )


def check_populations(degree, classes):
    n = classes["accepted"].size
    assert n == CASES_PER_DEGREE
    assert classes["accepted"].mean() >= MIN_ACCEPTED, (degree, classes["accepted"].mean())
    residual = classes["residual_depth_negative"] | classes["residual_colour_negative"]
    for name, mask in list(classes.items()) + [("residual_clamped", residual)]:
        assert int(mask.sum()) >= MIN_CLASS, f"degree {degree}: class {name} holds {int(mask.sum())} cases"
    # `galpha >= 0.999999` (gaussianParticles.cuh:573) is NOT reachable: galpha = fminf(0.99f, .) (:528).  That branch is left to reading.
    return {k: int(v.sum()) for k, v in classes.items()}
