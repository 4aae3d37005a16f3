"""The pose gradient's definition (pose.pose_gradient_from_rows) against float64 autograd of the per-ray oracle, and the host
maths of a pose increment."""
import importlib

import numpy as np
import pytest
import torch

from tests import off_centre_cases
from tests.common import cams, pose, scenes

per_ray = importlib.import_module("oracle.per_ray_torch")

W, H, FX = 64, 48, 64.0


def _twist_case(sh_degree, plane=None):
    """scene_c1(300, 0) seen from (0.3, -0.2, -4) at 64 x 48: the loss <cotangent, rgba> of the float64 per-ray render, with the
    first-order world-axis twist (rho, phi) about the camera centre applied to the camera-space rays,
        o_c' = R rho + A o_c,   d_c' = A d_c,   A = R (I + [phi]x) R^T,   R world -> sensor,
    so that the world-space rays are c + rho + (I + [phi]x)(...) while the pose every other part of the render sees (culling, depth
    order, the colours' view direction) stays put.  Returns (autograd d loss / d (rho, phi) at 0, activated rows, gradient rows,
    sensor position)."""
    sc = scenes.scene_c1(300, 0)
    c2w = cams.look_at_c2w((0.3, -0.2, -4.0), (0.0, 0.0, 0.0))
    tq = pose.sensor_pose_from_c2w(c2w).T_world_sensors[0]
    ro, rd = cams.pinhole_rays(W, H, FX, FX)
    if plane is not None:      # rays that do not start at the sensor position: the twist about the camera centre moves their origins too
        ro = off_centre_cases.origin_plane(plane, W, H)
    K = cams.pinhole_intrinsics_dict(W, H, FX, FX)
    cam = dict(model="pinhole", principal_point=K["principal_point"], focal_length=K["focal_length"], pose_start=tq)
    dt = torch.float64
    params = {k: torch.tensor(np.asarray(sc[k], np.float64), dtype=dt, requires_grad=k in ("positions", "rotation"))
              for k in ("positions", "rotation", "scale", "density", "features")}
    R, _, _, cam_pos = per_ray.pose_matrices(tq, dt)
    rho = torch.zeros(3, dtype=dt, requires_grad=True)
    phi = torch.zeros(3, dtype=dt, requires_grad=True)
    z = torch.zeros((), dtype=dt)
    skew = torch.stack([torch.stack([z, -phi[2], phi[1]]), torch.stack([phi[2], z, -phi[0]]), torch.stack([-phi[1], phi[0], z])])
    A = R @ (torch.eye(3, dtype=dt) + skew) @ R.T
    o_c = torch.as_tensor(ro, dtype=dt).reshape(-1, 3) @ A.T + R @ rho
    d_c = torch.as_tensor(rd, dtype=dt).reshape(-1, 3) @ A.T
    rgba, _, _ = per_ray.render_per_ray(cam, tq, W, H, params, o_c, d_c, sh_degree=sh_degree, dtype=dt)
    cot = torch.as_tensor(np.random.default_rng(1).standard_normal((H * W, 4)), dtype=dt)
    (rgba * cot).sum().backward()
    auto = torch.cat([rho.grad, phi.grad])
    act = torch.cat([params["positions"], params["density"], params["rotation"], params["scale"]], 1).detach()
    grad = torch.zeros_like(act)
    grad[:, 0:3] = params["positions"].grad
    grad[:, 4:8] = params["rotation"].grad
    return auto, act, grad, cam_pos


@pytest.mark.parametrize("sh_degree", [3, 0])
def test_reduction_of_the_gaussian_gradients_is_the_gradient_of_a_camera_twist(sh_degree):
    """d loss / d rho = -F and d loss / d phi = -M to 1e-7 of the largest component (measured: 1.2e-9; the slack is for another
    BLAS), and the quaternion torque is needed for it (without it the same comparison misses the bar)."""
    auto, act, grad, cam_pos = _twist_case(sh_degree)
    got = -pose.pose_gradient_from_rows(act, grad, cam_pos)
    assert got.dtype == torch.float64 and tuple(got.shape) == (6,)
    scale = float(auto.abs().max())
    assert scale > 0
    err = float((got - auto).abs().max()) / scale
    no_torque = -pose.pose_gradient_from_rows(act, grad, cam_pos, torque=False)
    err_no_torque = float((no_torque - auto).abs().max()) / scale
    print(f"[pose identity, SH degree {sh_degree}] autograd {auto.tolist()} error {err:.3e} of the largest component; "
          f"without the torque term {err_no_torque:.3e}")
    assert err <= 1e-7, err
    assert err_no_torque > 1e-7, err_no_torque   # the case is not vacuous: the torque term carries part of the answer
    # the translation part does not involve the torque at all
    assert torch.equal(no_torque[:3], got[:3])


def test_reference_condition_of_the_gpu_bar_holds_on_the_cpu_case():
    """The GPU test's bar is 1e-5 x S_k with S_k = sum_i |term_ik|; it says something only while |ref_k| >= 1e-3 S_k."""
    _, act, grad, cam_pos = _twist_case(3)
    terms = pose.pose_gradient_terms(act, grad, cam_pos)
    ratio = terms.sum(0).abs() / terms.abs().sum(0)
    assert float(ratio.min()) >= 1e-3, ratio.tolist()


def test_zero_twist_leaves_the_matrix_bit_identical():
    c2w = np.asarray(cams.orbit_c2w(4.0, 37.0, 12.0), np.float64)
    c2w[0, 1] = -0.0   # a signed zero must survive as well
    out = pose.apply_pose_increment(c2w, np.zeros(6))
    assert out.dtype == np.float64 and out.tobytes() == c2w.tobytes()
    assert out is not c2w


@pytest.mark.parametrize("phi", [(0.0, 0.0, 0.0), (1e-9, -2e-9, 3e-9), (1e-4, 2e-4, -1e-4), (0.3, -0.2, 0.1), (2.0, 1.0, -2.5)])
def test_exp_is_orthonormal(phi):
    R = pose.so3_exp(phi)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14
    # first order: exp([phi]x) v = v + phi x v + O(|phi|^2) (|v| < 1; 1e-15: the rounding of the two float64 evaluations)
    v = np.array([0.3, -0.7, 0.2])
    th = float(np.linalg.norm(phi))
    assert np.abs(R @ v - (v + np.cross(phi, v))).max() <= th * th + 1e-15


def test_two_increments_compose_as_the_product_of_their_matrices():
    c2w = np.asarray(cams.orbit_c2w(4.0, 200.0, -20.0), np.float64)
    d1 = np.array([0.01, -0.02, 0.03, 0.02, -0.01, 0.015])
    d2 = np.array([-0.03, 0.01, 0.00, -0.005, 0.03, 0.01])
    out = pose.apply_pose_increment(pose.apply_pose_increment(c2w, d1), d2)
    assert np.abs(out[:3, :3] - pose.so3_exp(d2[3:]) @ pose.so3_exp(d1[3:]) @ c2w[:3, :3]).max() <= 1e-15
    assert np.abs(out[:3, 3] - (c2w[:3, 3] + d1[:3] + d2[:3])).max() <= 1e-15
    assert np.array_equal(out[3], [0.0, 0.0, 0.0, 1.0])
    dt, dr = pose.pose_difference(out, c2w)
    assert dt == pytest.approx(np.linalg.norm(d1[:3] + d2[:3]), rel=1e-12)
    assert 0.0 < dr < np.linalg.norm(d1[3:]) + np.linalg.norm(d2[3:]) + 1e-12
