"""Grouped binning of the lazy per-tile depth order (k_expand_grouped: every entry goes straight into its tile's slice, K6 orders
each tile by (depth, particle id)) against the full stable sort (GUT_OPT_LAZY_TILE_ORDER = 0): the same image, distances, hit
counts, tile ranges and traversal depths, walked lists that are prefixes of the oracle's fully sorted lists, the same gradients."""
import numpy as np
import pytest
import torch

from tests.common import cams, make_view, rel_l2, scenes, to_batch
from tests.test_gpu_parity import CASES, DEV, _check_ordered_ids, _oracle_inputs, _run_gpu, gut, oracle

pytestmark = pytest.mark.gpu

GRADS = ("positions", "rotation", "scale", "density", "features_albedo")


def _permute(sc, idx):
    n = len(sc["positions"])
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in sc.items()}


def _morton_order(sc):
    """Storage order of the trainer: Morton order of the positions (neighbouring Gaussians share their tiles)."""
    p = sc["positions"]
    q = ((p - p.min(0)) / np.maximum(np.ptp(p, 0), 1e-9) * 1023).astype(np.uint64)
    code = np.zeros(len(p), np.uint64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return np.argsort(code, kind="stable")


def _compare(sc, view, rgba_grad):
    W, H = view["W"], view["H"]
    model, d12, sph = _oracle_inputs(sc, 3)
    ref = oracle.forward(view["oracle_cam"], W, H, d12, sph, view["ro"], view["rd"], sh_degree=3)
    a = _run_gpu(sc, view, 3, rgba_grad=rgba_grad, model=model, lazy=False)
    ga = {k: getattr(model, k).grad.clone() for k in GRADS}
    model.zero_grad(set_to_none=True)
    b = _run_gpu(sc, view, 3, rgba_grad=rgba_grad, model=model, lazy=True)
    for key in ("pred_rgb", "pred_dist", "hits_count"):
        assert torch.equal(a["out"][key], b["out"][key]), key
    ra, rb = a["tracer"].tracer_wrapper, b["tracer"].tracer_wrapper
    for key in ("tile_ranges", "tile_traversed_fwd"):
        assert torch.equal(ra.debug_buffer(key), rb.debug_buffer(key)), key
    assert np.array_equal(rb.debug_buffer("tile_ranges").cpu().numpy().view(np.uint32).reshape(-1, 2), ref["tile_ranges"])
    _check_ordered_ids(rb, ref)
    for k, g in ga.items():
        assert rel_l2(getattr(model, k).grad.cpu().numpy(), g.cpu().numpy()) <= 1e-5, k
    return ref


@pytest.mark.parametrize("order", ["given", "morton"])
@pytest.mark.parametrize("name", ["c1_pinhole_128", "ragged_100x70", "fisheye_144x96", "inside_cloud", "dense_big_splats"])
def test_grouped_binning_matches_the_full_sort(name, order):
    """"given": random storage order, every workgroup's window spans most of the grid; "morton": the trainer's order, compact
    windows.  At these sizes (at most 81 tiles) every window fits its 1536 LDS bins: the entries outside a window (per-entry
    global atomics) come only from large footprints.  Windows that do not fit, and workgroups without one, are
    tests/test_gpu_capacity_edges.py."""
    mk, kind, W, H, (eye, tgt), kw = CASES[name]
    sc = mk()
    if order == "morton":
        sc = _permute(sc, _morton_order(sc))
    view = make_view(kind, W, H, cams.look_at_c2w(eye, tgt), **kw)
    view.setdefault("W", W)
    view.setdefault("H", H)
    _compare(sc, view, np.random.default_rng(5).normal(size=(H, W, 4)).astype(np.float32))


@pytest.mark.parametrize("copies", [2, 80, 700])
def test_exact_depth_ties(copies):
    """Clones: bit-equal depths in the same tiles, ordered by particle id like the stable sort.  700 faint copies of one
    Gaussian in front of the scene put more than 64 ties across the first selection's boundary (K6's id select) and make the
    next selection start inside the group (ties with the last entry taken)."""
    sc = scenes.scene_c1(600, 9)
    n = len(sc["positions"])
    front = int(np.argmin(sc["positions"][:, 2]))
    sc["density"] = np.array(sc["density"], copy=True)
    sc["density"][front] = 0.02
    idx = np.concatenate([np.arange(n), np.full(copies, front), np.arange(0, n, 7)])
    sc = _permute(sc, np.random.default_rng(1).permutation(idx))
    W = H = 96
    view = make_view("pinhole", W, H, cams.look_at_c2w((0, 0, -4), (0, 0, 0)), fx=96)
    view.setdefault("W", W)
    view.setdefault("H", H)
    ref = _compare(sc, view, np.random.default_rng(6).normal(size=(H, W, 4)).astype(np.float32))
    lens = ref["tile_ranges"][:, 1] - ref["tile_ranges"][:, 0]
    assert lens.max() > min(copies, 64)


def test_overflow_redo_with_grouped_binning():
    """A frame with more intersections than the capacity the handle sized from the frame before: the grouped binning drops the
    slots beyond it, the host redoes it with the real count, and the result equals a fresh full-sort render."""
    sc = _permute(scenes.scene_c1(3000, 31), _morton_order(scenes.scene_c1(3000, 31)))
    W, H = 128, 96
    far = make_view("pinhole", W, H, cams.look_at_c2w((0, 0, -14.0), (0, 0, 0)), fx=110.0)
    near = make_view("pinhole", W, H, cams.look_at_c2w((0, 0, -2.2), (0, 0, 0)), fx=110.0)
    model = _oracle_inputs(sc, 3)[0]
    tr = gut.Tracer({"render": {}})
    tr.render(model, to_batch(far, DEV), train=False)
    out = tr.render(model, to_batch(near, DEV), train=False)
    assert tr.tracer_wrapper.stats()["binning_overflows"] >= 1
    ref = gut.Tracer({"render": {}})
    ref.tracer_wrapper.set_lazy_tile_order(False)
    exp = ref.render(model, to_batch(near, DEV), train=False)
    for key in ("pred_rgb", "pred_dist", "hits_count"):
        assert torch.equal(out[key], exp[key]), key
    assert torch.equal(tr.tracer_wrapper.debug_buffer("tile_ranges"), ref.tracer_wrapper.debug_buffer("tile_ranges"))
