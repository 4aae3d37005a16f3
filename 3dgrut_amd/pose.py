"""Host-side camera pose math of the tracer boundary.

Mirrors what `Tracer.__create_camera_parameters` + `SensorPose3DModel.get_sensor_pose` do in the
reference (threedgut_tracer/tracer.py:60-151, 373-383): camera-to-world 4x4 -> world-to-sensor
translation + unit quaternion in XYZW order, float32, start pose == end pose, timestamps [0, 1].
Pinned by tests/golden/pose_golden.npz (generated from the reference's own Python).
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class SensorPose3D:
    T_world_sensors: list  # two [t(3), q(xyzw)] float32 arrays (start, end)
    timestamps_us: list


def _world_to_view(c2w34):
    # the reference inverts C2W in float64, rebuilds C2W and inverts again (tracer.py:75-85, 376-383)
    c2w = np.concatenate((np.asarray(c2w34, np.float64)[:3, :4], np.zeros((1, 4))))
    c2w[3, 3] = 1.0
    w2c = np.linalg.inv(c2w)
    rt = np.zeros((4, 4))
    rt[:3, :3] = w2c[:3, :3]
    rt[:3, 3] = w2c[:3, 3]
    rt[3, 3] = 1.0
    rt = np.linalg.inv(np.linalg.inv(rt))
    return np.float32(rt)


def so3_matrix_to_quat_xyzw(R):
    """Largest-diagonal/trace branch selection as tracer.py:88-136, float32 arithmetic."""
    R = np.asarray(R, np.float32)
    dec = np.array([R[0, 0], R[1, 1], R[2, 2], np.float32(0)], np.float32)
    dec[3] = dec[:3].sum(dtype=np.float32)
    choice = int(np.argmax(dec))
    q = np.empty(4, np.float32)
    if choice != 3:
        i = choice
        j = (i + 1) % 3
        k = (j + 1) % 3
        q[i] = np.float32(1) - dec[3] + np.float32(2) * R[i, i]
        q[j] = R[j, i] + R[i, j]
        q[k] = R[k, i] + R[i, k]
        q[3] = R[k, j] - R[j, k]
    else:
        q[0] = R[2, 1] - R[1, 2]
        q[1] = R[0, 2] - R[2, 0]
        q[2] = R[1, 0] - R[0, 1]
        q[3] = np.float32(1) + dec[3]
    return q / np.float32(np.sqrt((q * q).sum(dtype=np.float32)))


def sensor_pose_from_c2w(T_to_world) -> SensorPose3D:
    rt = _world_to_view(np.asarray(T_to_world).reshape(4, 4))
    tq = np.concatenate([rt[:3, 3], so3_matrix_to_quat_xyzw(rt[:3, :3])]).astype(np.float32)
    return SensorPose3D(T_world_sensors=[tq, tq.copy()], timestamps_us=[0, 1])


# ----------------------------------------------------------------------------------------------------
# Camera-pose gradient and pose increments (pose refinement)
# ----------------------------------------------------------------------------------------------------
def pose_gradient_terms(act12, grad12, cam_pos, torque=True):
    """Per-row terms [N,6] (float64, on the rows' device) of the pose-gradient reduction: columns 0..2 g_mu, columns 3..5
    (mu - c) x g_mu + tau with tau_k = 1/2 g_q . ((0, e_k) (x) q).  act12 / grad12: [N,>=8] rows in density12 layout (pos3, density,
    quat wxyz, scale3): the activated parameters and the gradient with respect to them, as the backward leaves it; cam_pos: the
    sensor position [3].  torque=False leaves tau out (tests: the term is required)."""
    import torch
    a = torch.as_tensor(act12).to(torch.float64)
    g = torch.as_tensor(grad12, device=a.device).to(torch.float64)
    c = torch.as_tensor(cam_pos, device=a.device).to(torch.float64).reshape(3)
    g_mu, g_q = g[:, 0:3], g[:, 4:8]
    moment = torch.linalg.cross(a[:, 0:3] - c, g_mu, dim=1)
    if torque:
        w, x, y, z = a[:, 4:8].unbind(1)
        # (0, e_k) (x) q in wxyz order, k = x, y, z
        ex = torch.stack([-x, w, -z, y], 1)
        ey = torch.stack([-y, z, w, -x], 1)
        ez = torch.stack([-z, -y, x, w], 1)
        moment = moment + 0.5 * torch.stack([(g_q * ex).sum(1), (g_q * ey).sum(1), (g_q * ez).sum(1)], 1)
    return torch.cat([g_mu, moment], 1)


def pose_gradient_from_rows(act12, grad12, cam_pos, torque=True):
    """The definition of the pose gradient: (F, M) as a float64 [6] tensor,
        F = sum_i g_mu_i,    M = sum_i (mu_i - c) x g_mu_i + tau_i.
    For the camera perturbation c' = c + rho, R_c2w' = exp([phi]x) R_c2w (a world-axis twist, the rotation about the camera centre):
    dL/d rho = -F and dL/d phi = -M.  This is the gradient the backward defines: the per-ray evaluation is differentiated, the
    projection (tile membership) is not, and the colours' view direction is held fixed as it is for the position gradient.  It
    holds for a view with ONE pose (pose_start == pose_end).  Rows without a gradient contribute nothing, so the dense [N,12]
    gradient of a backward may be passed as it is."""
    return pose_gradient_terms(act12, grad12, cam_pos, torque).sum(0)


def so3_exp(phi):
    """exp([phi]x) as a float64 3x3 rotation matrix (Rodrigues; the small-angle forms keep it orthonormal to rounding)."""
    phi = np.asarray(phi, np.float64).reshape(3)
    theta = float(np.sqrt(phi @ phi))
    K = np.array([[0.0, -phi[2], phi[1]], [phi[2], 0.0, -phi[0]], [-phi[1], phi[0], 0.0]])
    if theta < 1e-5:
        a, b = 1.0 - theta * theta / 6.0, 0.5 - theta * theta / 24.0
    else:
        a, b = np.sin(theta) / theta, 2.0 * np.sin(0.5 * theta) ** 2 / (theta * theta)
    return np.eye(3) + a * K + b * (K @ K)


def apply_pose_increment(c2w, delta6):
    """Camera-to-world 4x4 (float64) after the increment (d_rho, d_phi): c += d_rho, R <- exp([d_phi]x) R.  A zero increment
    returns the matrix bit for bit."""
    out = np.array(c2w, np.float64, copy=True).reshape(4, 4)
    d = np.asarray(delta6, np.float64).reshape(6)
    if not d.any():
        return out
    out[:3, :3] = so3_exp(d[3:6]) @ out[:3, :3]
    out[:3, 3] = out[:3, 3] + d[0:3]
    return out


def pose_difference(c2w_a, c2w_b):
    """(|centre_a - centre_b|, rotation angle between the two in radians) of two camera-to-world matrices."""
    a, b = np.asarray(c2w_a, np.float64).reshape(4, 4), np.asarray(c2w_b, np.float64).reshape(4, 4)
    dr = a[:3, :3] @ b[:3, :3].T
    s = 0.5 * np.array([dr[2, 1] - dr[1, 2], dr[0, 2] - dr[2, 0], dr[1, 0] - dr[0, 1]])
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(dr) - 1.0)))
