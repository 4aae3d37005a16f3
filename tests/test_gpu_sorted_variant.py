"""The sorted variant of the compositor (render.splat.k_buffer_size = K; gut_render_sorted.hip) held to the standard of the default
path: every pixel outside COLOUR_TOL, or with another hit count, must be explained by the k-buffer oracle's own decision margins
(hit / no-hit, hit-distance range, termination, ORDER) and stay within its own flip budget; every gradient row must sit inside its
own fp32-noise and flip budget (oracle.render_kbuffer / oracle.kbuffer_backward; the model's constants are measured on the CPU by
tests/test_cpu_oracle.py::test_two_fp32_evaluations_measure_the_kbuffer_model and, per case, tests/test_cpu_sorted_cases.py).

The cases (tests/sorted_cases.py) reach the kernels' edges: K = 1 and K = 16 (`first = kKMax - K` = 15 and 0: the two ends of
kb_front, kb_insert and the drain), lists of 255 ... 3336 entries on one tile (up to 14 stagings with the k-buffer carried across the
reloads; hits of an earlier chunk composited after hits of a later one), rays that terminate with hits pending, clones whose order
only the insertion rule decides, hit distances of exactly zero (all the range test against tmin rejects inside the scene box).  The inputs are the activated [N,12] / [N,48] rows themselves (SplatRaster.trace / trace_bwd), so
the oracle's preconditions hold bit for bit on the device; the gradients are compared in that activated space."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import sorted_cases as sc
from tests.common import GRAD_BLOCKS, ROW_FLIP_BOUND, check_colour_outliers, check_gradient_rows, to_batch

pytestmark = pytest.mark.gpu

gut = importlib.import_module("3dgrut_amd")
oracle = importlib.import_module("oracle.oracle")
DEV = "cuda:0"

CASES = {
    **{f"single_tile_{n}": (lambda n=n: sc.single_tile(n)) for n in (255, 256, 257, 513, 1025)},
    "terminating_deep_list": sc.terminating_deep_list,
    "geometry_clones": sc.geometry_clones,
    "rays_from_a_centre_plane": sc.rays_from_a_centre_plane,
    **{name: (lambda name=name: sc.existing(name)) for name in sc.EXISTING},
}
BACKWARD_CASES = [n for n in CASES if n not in ("single_tile_255", "single_tile_256")]


def run_sorted(case, K, rgba_grad=None, dist_grad=None, conf=None, reference_backward=False, active_sh=None):
    """One forward (and, with rgba_grad, one backward) of the case's activated rows on a fresh handle with k_buffer_size = K."""
    render = dict(conf or {})
    render["splat"] = dict(render.get("splat", {}), k_buffer_size=K, sorted_reference_backward=reference_backward)
    tr = gut.Tracer({"render": render})
    raster = tr.tracer_wrapper
    view = case["view"]
    sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
    ro, rd = torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous()
    d12, sph = torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV)
    cam = (ro, rd, None, sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0], poses.T_world_sensors[1])
    sh = case["sh_degree"] if active_sh is None else active_sh
    rgba, dist, hits, _ = raster.trace(0, sh, d12, sph, *cam)
    out = dict(rgba=rgba.cpu().numpy(), dist=dist.cpu().numpy(), hits=hits.cpu().numpy())
    if rgba_grad is not None:
        g12, g48 = raster.trace_bwd(0, sh, d12, sph, *cam, rgba, torch.as_tensor(rgba_grad, device=DEV), dist,
                                    None if dist_grad is None else torch.as_tensor(dist_grad, device=DEV))
        out.update(g12=g12.cpu().numpy(), g48=g48.cpu().numpy())
    return out


def check_sorted_forward(case, K, got, label):
    """Every pixel against the k-buffer oracle's margins and its own budget (colour, opacity, hit distance, hit count)."""
    kb = sc.kbuffer(case, K, ROW_FLIP_BOUND)
    return check_colour_outliers(got["rgba"], got["hits"], kb, kb["margins"], label=label, dist_gpu=got["dist"], budget=kb["pixel_budget"])


_BACKWARD = {}


def oracle_backward(case, K, rgba_grad, dist_grad, reference_undo_colour=False):
    key = (case["name"], K, dist_grad is not None, reference_undo_colour, rgba_grad.tobytes()[:64])
    if key not in _BACKWARD:
        _BACKWARD[key] = oracle.kbuffer_backward(case["view"]["oracle_cam"], case["ref"], K, rgba_grad, dist_grad, params=case["params"](),
                                                 flip_bound=ROW_FLIP_BOUND, reference_undo_colour=reference_undo_colour)
    return _BACKWARD[key]


def check_sorted_backward(case, K, got, rgba_grad, dist_grad, label, reference_undo_colour=False):
    """Every row of every block against its own bound; rows the oracle composites on no pixel, in neither of its walks, exactly zero."""
    ob = oracle_backward(case, K, rgba_grad, dist_grad, reference_undo_colour)
    budget = ob["budget"]
    rows = {}
    for j, (block, sl) in enumerate(GRAD_BLOCKS):
        rows[block] = check_gradient_rows(got["g12"][:, sl], ob["dens_g"][:, sl], f"{label}/{block}", budget[:, j], budget[:, 5 + j])
    y = math.sqrt((case["sh_degree"] + 1) ** 2 / (4 * math.pi))
    rows["sh"] = check_gradient_rows(got["g48"], ob["sph_g"], f"{label}/sh", budget[:, 4] * y, budget[:, 9] * y)
    never = (np.abs(ob["dens_g"]).max(1) == 0) & (np.abs(ob["sph_g"]).max(1) == 0) & (budget[:, :5].max(1) == 0)
    assert not np.abs(got["g12"][never]).max(initial=0.0) and not np.abs(got["g48"][never]).max(initial=0.0), \
        f"{label}: rows of Gaussians the oracle never composites got a gradient"
    assert float(np.abs(got["g12"][:, 11]).max()) == 0.0
    return rows


def _grads(case, seed, with_dist_grad):
    rng = np.random.default_rng(seed)
    H, W = case["H"], case["W"]
    rg = rng.normal(size=(H, W, 4)).astype(np.float32)
    dg = (0.1 * rng.normal(size=(H, W, 1))).astype(np.float32) if with_dist_grad else None
    return rg, dg


@pytest.mark.parametrize("K", [1, 2, 4, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_sorted_forward_per_pixel(name, K):
    case = CASES[name]()
    got = run_sorted(case, K)
    check_sorted_forward(case, K, got, f"{name}/K={K}")
    if K == 16:
        # the forward has no atomics: two runs give identical bits
        again = run_sorted(case, K)
        for key in ("rgba", "dist", "hits"):
            assert np.array_equal(got[key].view(np.uint32), again[key].view(np.uint32)), f"{name}: {key} differs between two runs"
    if K == 1 and name == "c1_pinhole_128":
        # K = 1 composites in list order: it must agree with the unsorted compositor
        tr = gut.Tracer({"render": {}})
        view = case["view"]
        sensor, poses = gut.Tracer.create_camera_parameters(to_batch(view, DEV))
        rgba0 = tr.tracer_wrapper.trace(0, 3, torch.as_tensor(case["d12"], device=DEV), torch.as_tensor(case["sph"], device=DEV),
                                        torch.as_tensor(view["ro"], device=DEV).contiguous(), torch.as_tensor(view["rd"], device=DEV).contiguous(),
                                        None, sensor, poses.timestamps_us[0], poses.timestamps_us[1], poses.T_world_sensors[0],
                                        poses.T_world_sensors[1])[0].cpu().numpy()
        assert np.abs(got["rgba"][..., :3] - rgba0[..., :3]).max() <= 2e-5


def test_clone_order_is_the_insertion_rules():
    """geometry_clones and its reversed twin: the two images differ by up to 0.2 on the clones' pixels (tests/test_cpu_sorted_cases.py),
    and the device follows the oracle on both at the flat tolerance: the clones' comparisons have no margin and no budget."""
    for reverse in (False, True):
        case = sc.geometry_clones(reverse)
        for K in (2, 16):
            rep = check_sorted_forward(case, K, run_sorted(case, K), f"{case['name']}/K={K}")
            assert rep["outliers"] <= 2


@pytest.mark.parametrize("with_dist_grad", [False, True])
@pytest.mark.parametrize("K", [1, 8, 16])
@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_sorted_backward_per_row(name, K, with_dist_grad):
    case = CASES[name]()
    rg, dg = _grads(case, 5, with_dist_grad)
    got = run_sorted(case, K, rg, dg)
    check_sorted_forward(case, K, got, f"{name}/K={K}")
    check_sorted_backward(case, K, got, rg, dg, f"{name}/K={K}/dist={int(with_dist_grad)}")


@pytest.mark.parametrize("reference_backward", [False, True])
def test_sorted_backward_forms_on_negative_colours(reference_backward):
    """Both values of sorted_reference_backward on the scene with negative colour channels, where the reference's own un-do form and
    the exact derivative differ (tests/test_gpu_parity.py::test_sorted_variant_reference_backward shows by how much)."""
    case = sc.existing("c1_pinhole_128", negative_colours=True)
    assert (case["ref"]["feat"][case["ref"]["tiles_count"] > 0] < 0).any()
    K = 8
    rg, _ = _grads(case, 8, False)
    got = run_sorted(case, K, rg, None, reference_backward=reference_backward)
    check_sorted_backward(case, K, got, rg, None, f"negative colours/reference_backward={reference_backward}", reference_undo_colour=reference_backward)


def _toggle(name):
    toggles = importlib.import_module("tests.test_gpu_parity").TOGGLES
    return toggles[name]


CONFIGS = {
    "kernel_degree_3": lambda: _toggle("kernel_degree_3") + (None,),
    "kernel_degree_5": lambda: _toggle("kernel_degree_5") + (None,),
    "kernel_degree_8": lambda: _toggle("kernel_degree_8") + (None,),
    "thresholds": lambda: _toggle("thresholds") + (None,),                # particle_kernel_max_alpha = 0.9
    "thresholds_loose": lambda: _toggle("thresholds_loose") + (None,),    # ... 0.999
    "hitcounts_off": lambda: _toggle("hitcounts_off") + (None,),
    "sh_degree_1": lambda: ({}, {}, 1),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_sorted_variant_configurations(config):
    """k_buffer_size = 8 together with the configuration keys that reach the sorted kernels: forward per pixel, backward per row
    (with a hit-distance gradient), and the key must change the oracle's result."""
    conf, overrides, sh = CONFIGS[config]()
    K = 8
    base = sc.existing("c1_pinhole_128")
    if sh is None:
        case = sc.existing("c1_pinhole_128", **overrides)
    else:
        case = sc._finish(f"c1_pinhole_128/sh={sh}", base["d12"], base["sph"], base["view"], base["W"], base["H"], sh_degree=sh)
    kb, kb0 = sc.kbuffer(case, K), sc.kbuffer(base, K)
    assert not (np.array_equal(kb["rgba"], kb0["rgba"]) and np.array_equal(kb["hits"], kb0["hits"])), f"{config} changes nothing: the case does not test it"
    rg, dg = _grads(case, 17, True)
    got = run_sorted(case, K, rg, dg, conf=conf)
    check_sorted_forward(case, K, got, f"c1_pinhole_128/{config}/K={K}")
    if config == "hitcounts_off":
        assert not got["hits"].any()
    check_sorted_backward(case, K, got, rg, dg, f"c1_pinhole_128/{config}/K={K}")
    if sh is not None:
        nc = (sh + 1) ** 2
        assert not got["g48"][:, 3 * nc:].any(), "coefficients above the active degree must get zero gradient"
