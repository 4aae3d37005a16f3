"""The bilateral grids of DESIGN.md §21 without a GPU: the float32 restatement is held to the float64 definition by an a-priori
bound, the case table of the GPU file meets its preconditions, the adjoint has its symmetries as bits, and the host logic — the
config block and its refusals, the flags, the checkpoint, the bindings and their refusals — says what §21 says."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

from tests import bilateral_reference as br
from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

_capi = importlib.import_module("3dgrut_amd._capi")
bilateral = importlib.import_module("3dgrut_amd.bilateral")
losses = importlib.import_module("3dgrut_amd.losses")
native = importlib.import_module("3dgrut_amd.native")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")

F = np.float32
LAMBDA_TV = 10.0
CPU_CASES = [name for name in br.CASES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- (a) against (b) ----
@pytest.mark.parametrize("name", CPU_CASES)
def test_the_restatement_stays_within_the_bound_of_the_definition(name):
    """Every output element of (a) within n 2^-24 sum |terms| of (b): n is the number of roundings on the element's longest path
    through §21's order (N_SLICE = 23, N_IMAGE = 23, N_ALPHA = 27, N_GRID = 13, N_TV = 9, derived line by line in
    tests/bilateral_reference.py), sum |terms| the element's expression with every operand replaced by its absolute value.  The grid
    gradient adds half a unit 2^-s per product it received (the rounding to an integer) and, with the TV term, that term's own
    bound.  The image gradient is compared where both references take the same level piece and the same side of the clamp (the
    derivative by the guidance is discontinuous there; everything else is continuous across pieces).  Largest ratios observed over
    the cases: slice 0.063, image gradient 0.091, grid gradient 0.383."""
    c = br.case(name)
    shape = c["grid"].shape[1:]
    mag = br.magnitudes(c["rgba"], c["background"], c["grid"], c["out_grad"], LAMBDA_TV)
    out32 = br.slice32(c["rgba"], c["background"], c["grid"])
    out64 = br.slice64(c["rgba"], c["background"], c["grid"])
    assert np.array_equal(_bits(out32[..., 3]), _bits(c["rgba"][..., 3]))          # alpha passes through
    finite = np.isfinite(out64).all(axis=-1)
    assert np.array_equal(np.isfinite(out32[..., :3]).all(axis=-1), finite)
    r_slice = float((np.abs(out32[..., :3] - out64)[finite] / (br.N_SLICE * br.U * mag["out"][finite])).max())

    image32, grid32 = br.backward32(c["rgba"], c["background"], c["grid"], c["out_grad"], LAMBDA_TV)
    image64, grid64 = br.backward64(c["rgba"], c["background"], c["grid"], c["out_grad"], LAMBDA_TV)
    p = br.pixels32(c["rgba"], c["background"], shape)
    z64, inside64 = br.branches64(c["rgba"], c["background"], shape)
    same = ((z64 == p["z"][:, 0]) & (inside64 == p["inside"])).reshape(finite.shape) & finite
    assert same.mean() >= (0.9 if name == "kink" else 0.995)                        # (the kink case sits ON the boundaries)
    n_image = np.array([br.N_IMAGE] * 3 + [br.N_ALPHA], dtype=np.float64)
    r_image = float((np.abs(image32 - image64)[same] / (n_image * br.U * mag["image"][same])).max())
    bound = br.N_GRID * br.U * mag["grid"] + 0.5 * mag["contributions"] * mag["unit"] + br.N_TV * br.U * mag["tv"]
    assert (bound > 0).all()
    r_grid = float((np.abs(grid32 - grid64) / bound).max())
    print(f"\n[bilateral {name}] ratio to the bound: slice {r_slice:.3f}, image gradient {r_image:.3f}, grid gradient {r_grid:.3f}; "
          f"same piece {same.mean():.4f}")
    assert r_slice <= 1.0 and r_image <= 1.0 and r_grid <= 1.0


# ---- the case table ----
def test_the_case_table_meets_its_preconditions():
    assert set(br.CASES) == {"edges", "edges_plane", "single_cell", "row", "column", "overflow", "kink", "shipped"}
    assert br.TABLE == _capi.BILATERAL_TABLE and br.TILE == _capi.BILATERAL_TILE
    for name, (H, W, triple, bg) in br.CASES.items():
        c = br.case(name)
        shape = br.grid_shape(triple)
        assert c["grid"].shape == (12,) + shape and c["rgba"].shape == (H, W, 4) and c["out_grad"].shape == (H, W, 4)
        assert (np.ndim(c["background"]) == 0) == (bg != "plane")
        p = br.pixels32(c["rgba"], c["background"], shape)
        assert p["inside"].any() and (~p["inside"]).any(), name                     # pixels on both sides of `inside`
        assert (p["g"] <= 0).any() and (p["g"] >= 1).any(), name
        if name == "overflow":
            assert br.footprint(name) > br.TABLE                                    # the direct route
        else:
            assert br.footprint(name) <= br.TABLE, name                             # the LDS table
    assert br.CASES["edges"][0] % br.TILE and br.CASES["edges"][1] % br.TILE        # partial tiles, more than one workgroup
    assert br.CASES["edges"][1] > 2 * br.TILE
    assert br.CASES["row"][0] == 1 and br.CASES["column"][1] == 1
    assert br.scales(1, 40, 3, 3) == (F(2) / F(39), F(0)) and br.scales(40, 1, 3, 3) == (F(0), F(2) / F(39))
    # single cell: every pixel into the same 12 sums
    p = br.pixels32(br.case("single_cell")["rgba"], 1.0, (1, 1, 1))
    assert not p["cell"].any()
    # the shipped grid needs the 3 x 3 footprint the table was sized for
    assert br.footprint("shipped") == 3 * 3 * 8 * 12


def test_the_kink_case_sits_on_the_boundaries():
    """Luminances exactly 0 and exactly 1 (outside: the clamp's side), sz exactly k for every interior level (inside, fz = 0, the
    piece to the right), below 0, above 1, and NaN (counts as 0, outside)."""
    c = br.case("kink")
    L = c["grid"].shape[1]
    p = br.pixels32(c["rgba"], c["background"], c["grid"].shape[1:])
    g, sz = p["g"], (np.where(np.isnan(p["g"]), F(0), np.clip(p["g"], F(0), F(1))) * F(L - 1)).astype(F)
    assert (g == 0).sum() >= 6 and (g == 1).sum() >= 6 and (g < 0).any() and (g > 1).any() and np.isnan(g).sum() >= 6
    assert not p["inside"][(g == 0) | (g == 1) | np.isnan(g)].any()
    for k in range(1, L - 1):
        at = p["inside"] & (sz == F(k))
        assert at.sum() >= 6, k
        assert (p["z"][at, 0] == k).all() and (p["wz"][at, 1] == 0).all() and (p["wz"][at, 0] == 1).all()
    nan = np.isnan(g)
    assert (p["z"][nan, 0] == 0).all()
    out = br.slice32(c["rgba"], c["background"], c["grid"]).reshape(-1, 4)
    assert np.isnan(out[nan, :3]).all() and np.isfinite(out[~nan]).all()
    image, grid = br.backward32(c["rgba"], c["background"], c["grid"], c["out_grad"])
    assert np.isfinite(image).all() and np.isfinite(grid).all()                    # a NaN colour poisons neither gradient


# ---- properties of the restatement ----
def _identity(shape):
    G = np.zeros((12,) + tuple(shape), dtype=F)
    G[0], G[5], G[10] = 1.0, 1.0, 1.0
    return G


@pytest.mark.parametrize("name", ["edges", "edges_plane", "shipped"])
def test_an_identity_grid_changes_nothing(name):
    """out = comp within the slice's bound (the eight weights sum to 1 up to their roundings), and the image gradient IS g'
    (A = I exactly where it matters: 1 g'_j + 0 + 0, and D = 0 because every level holds the same transform)."""
    c = br.case(name)
    G = _identity(c["grid"].shape[1:])
    p = br.pixels32(c["rgba"], c["background"], G.shape[1:])
    out = br.slice32(c["rgba"], c["background"], G)
    mag = br.magnitudes(c["rgba"], c["background"], G)
    comp64, _ = br.comp64(c["rgba"], c["background"])
    assert (np.abs(out[..., :3] - comp64) <= br.N_SLICE * br.U * mag["out"]).all()
    A = br.gather32(G, p)
    assert np.abs(A - _identity((1, 1, 1)).reshape(12)).max() <= 4 * 2.0 ** -24
    image, _ = br.backward32(c["rgba"], c["background"], G, c["out_grad"])
    bound = br.N_IMAGE * br.U * br.magnitudes(c["rgba"], c["background"], G, c["out_grad"])["image"][..., :3]
    assert (np.abs(image[..., :3].astype(np.float64) - c["out_grad"][..., :3]) <= bound).all()
    exact = ((A[:, 0] == 1) & (A[:, 5] == 1) & (A[:, 10] == 1)).reshape(image.shape[:2])   # the weights summed to 1 without an error
    assert exact.mean() > 0.2
    assert np.array_equal(image[..., :3][exact], c["out_grad"][..., :3][exact])


@pytest.mark.parametrize("name", ["edges_plane", "overflow", "kink"])
def test_symmetries_of_the_adjoint(name):
    c = br.case(name)
    image, grid = br.backward32(c["rgba"], c["background"], c["grid"], c["out_grad"])
    image_n, grid_n = br.backward32(c["rgba"], c["background"], c["grid"], -c["out_grad"])
    # (0 - x: the exact negation of every non-zero value, and +0 where the sum is zero, which the conversion writes as +0)
    assert np.array_equal(_bits(grid_n), _bits(F(0) - grid))
    assert np.array_equal(image_n, -image)
    for m in (-20, 3, 60):
        image_m, grid_m = br.backward32(c["rgba"], c["background"], c["grid"], np.ldexp(c["out_grad"], m))
        assert np.array_equal(_bits(grid_m), _bits(np.ldexp(grid, m))), m
        assert np.array_equal(_bits(image_m), _bits(np.ldexp(image, m))), m
    bad, holes = br.non_finite_cotangent(c["out_grad"])
    assert not np.isfinite(bad[..., :3]).all() and (holes[..., :3] == 0).any()
    a, b = br.backward32(c["rgba"], c["background"], c["grid"], bad), br.backward32(c["rgba"], c["background"], c["grid"], holes)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    zero = br.backward32(c["rgba"], c["background"], c["grid"], np.zeros_like(c["out_grad"]))
    assert not _bits(zero[1]).any()                                                 # +0 everywhere


def test_the_tv_term():
    """lambda_tv 0 adds nothing (the bits of the sums' conversion); an axis of length 1 contributes nothing; a constant grid has no
    TV gradient; the float32 term follows the float64 one."""
    rng = np.random.default_rng(5)
    for shape in ((2, 3, 4), (1, 3, 4), (2, 1, 1), (1, 1, 1)):
        G = rng.standard_normal((12,) + shape).astype(F)
        grad = rng.standard_normal(G.shape).astype(F)
        assert np.array_equal(_bits(br.finish32(grad, G, 0.0)), _bits(grad))
        Gt = torch.from_numpy(G.astype(np.float64)).requires_grad_(True)
        tv = losses.bilateral_total_variation(Gt)
        want = torch.autograd.grad(tv, Gt)[0].numpy() if tv.requires_grad else np.zeros(G.shape)
        got = br.tv_term32(G, 3.0)
        assert np.abs(got - 3.0 * want).max() <= br.N_TV * br.U * 3.0 * 4.0 * np.abs(G).max(), shape
        assert not br.tv_term32(np.ones_like(G), 3.0).any()
    assert float(losses.bilateral_total_variation(torch.ones(12, 1, 1, 1))) == 0.0
    G = torch.zeros(12, 2, 1, 1)
    G[:, 1] = 2.0
    assert float(losses.bilateral_total_variation(G)) == 4.0                        # one axis, every squared difference 4


def test_the_definition_in_torch():
    """losses.bilateral_slice: any dtype, [H,W,3] and [1,H,W,3]; identity grid -> comp; the gradient reaches both operands."""
    c = br.case("edges")
    comp = torch.from_numpy(br.comp64(c["rgba"], c["background"])[0])
    G = torch.from_numpy(c["grid"].astype(np.float64))
    out = losses.bilateral_slice(comp, G)
    assert out.dtype == torch.float64 and out.shape == comp.shape
    assert torch.equal(losses.bilateral_slice(comp[None], G)[0], out)
    assert losses.bilateral_slice(comp.float(), G.float()).dtype == torch.float32
    assert float((losses.bilateral_slice(comp, torch.from_numpy(_identity(G.shape[1:]).astype(np.float64))) - comp).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="grid must be"):
        losses.bilateral_slice(comp, G[:11])
    with pytest.raises(ValueError, match="comp must be"):
        losses.bilateral_slice(comp[..., :2], G)
    # a finite difference through the guidance, inside a piece
    x = torch.tensor([[[0.31, 0.42, 0.27]]], dtype=torch.float64, requires_grad=True)
    Gs = torch.from_numpy(br.case("kink")["grid"].astype(np.float64))
    (losses.bilateral_slice(x, Gs)[0, 0, 1]).backward()
    h = 1e-6
    e = torch.zeros_like(x)
    e[0, 0, 1] = h
    with torch.no_grad():
        fd = (losses.bilateral_slice(x + e, Gs)[0, 0, 1] - losses.bilateral_slice(x - e, Gs)[0, 0, 1]) / (2 * h)
    assert abs(float(x.grad[0, 0, 1]) - float(fd)) <= 1e-7


def test_host_grids():
    """BilateralGrids on the host: identity at the start, begin() hands out a view with the TV weight, apply() is the definition, and
    end() is the restatement's Adam step, per view."""
    g = bilateral.BilateralGrids(3, (4, 3, 2), "cpu", lr=0.01, lambda_tv=2.5)
    assert tuple(g.params.shape) == (3, 12, 2, 3, 4) and g.shape == (4, 3, 2) and g.num_views == 3
    assert np.array_equal(g.params[1].numpy(), _identity((2, 3, 4)))
    assert [g.active(s) for s in (0, 5)] == [True, True]
    w = bilateral.BilateralGrids(1, (1, 1, 1), "cpu", start_iteration=2, end_iteration=4)
    assert [w.active(s) for s in range(5)] == [False, False, True, True, False]

    class B:
        pass
    batch = g.begin(1, B())
    assert batch.bilateral_grid.data_ptr() == g.params[1].data_ptr() and batch.bilateral_lambda_tv == 2.5
    rgba = torch.rand((5, 7, 4), generator=torch.Generator().manual_seed(1))
    out = g.apply(1, rgba, 1.0)
    comp = rgba[..., :3] + 1.0 * (1.0 - rgba[..., 3:])
    assert float((out[..., :3] - comp).abs().max()) <= 1e-6 and torch.equal(out[..., 3], rgba[..., 3])
    grad = torch.randn(g.params[1].shape, generator=torch.Generator().manual_seed(2))
    want = br.adam32(grad.numpy(), g.params[1].numpy(), g.m[1].numpy(), g.v[1].numpy(), 0, 0.01, 0.9, 0.999, 1e-15)
    g.end(1, grad)
    assert g.counts.tolist() == [0, 1, 0]
    assert np.abs(g.params[1].numpy() - want[0]).max() <= 1e-7 and np.array_equal(g.params[0].numpy(), _identity((2, 3, 4)))
    sm = g.summary()
    assert sm["grid"] == [4, 3, 2] and sm["mean_tv"] > 0 and abs(sm["mean_gain"] - 1.0) < 0.01
    for bad in ((0, 3, 2), (4, 3), (4, 3, 257), (4.0, 3, 2)):
        with pytest.raises(ValueError, match="shape must be three integers"):
            bilateral.BilateralGrids(1, bad, "cpu")
    with pytest.raises(ValueError, match="no views"):
        bilateral.BilateralGrids(0, (4, 3, 2), "cpu")
    with pytest.raises(ValueError, match="lambda_tv must be finite"):
        bilateral.BilateralGrids(1, (4, 3, 2), "cpu", lambda_tv=float("inf"))


# ---- host logic ----
def test_config_rules():
    blk = trainer_mod.resolve_config({})["bilateral"]
    assert blk == {"enabled": False, "grid": [16, 16, 8], "lr": 0.002, "lambda_tv": 10.0, "start_iteration": 0, "end_iteration": -1,
                   "beta1": 0.9, "beta2": 0.999, "eps": 1e-15} == bilateral.DEFAULTS
    ok = trainer_mod.resolve_config({"bilateral": {"enabled": True, "grid": [8, 4, 2], "lr": 0.0, "lambda_tv": 0.0, "end_iteration": 9}})
    assert ok["bilateral"]["enabled"] is True and ok["bilateral"]["grid"] == [8, 4, 2] and ok["bilateral"]["beta2"] == 0.999
    for override, words in (({"grid": [16, 16]}, "bilateral.grid must be three integers [Gw, Gh, L] in 1 .. 256, got [16, 16]"),
                            ({"grid": [16, 0, 8]}, "bilateral.grid must be three integers [Gw, Gh, L] in 1 .. 256, got [16, 0, 8]"),
                            ({"grid": [16, 16, 257]}, "bilateral.grid must be three integers [Gw, Gh, L] in 1 .. 256, got [16, 16, 257]"),
                            ({"grid": [16, 16, 8.0]}, "bilateral.grid must be three integers [Gw, Gh, L] in 1 .. 256, got [16, 16, 8.0]"),
                            ({"lr": -0.1}, "bilateral.lr must be finite and >= 0, got -0.1"),
                            ({"lambda_tv": float("inf")}, "bilateral.lambda_tv must be finite and >= 0, got inf"),
                            ({"lambda_tv": -1}, "bilateral.lambda_tv must be finite and >= 0, got -1"),
                            ({"beta1": 1.0}, "bilateral.beta1 must be in [0, 1), got 1.0"),
                            ({"enabled": 1}, "bilateral.enabled must be true or false, got 1"),
                            ({"start_iteration": -1}, "bilateral: start_iteration must be >= 0 and end_iteration >= 0, or -1 for the end of the run"),
                            ({"end_iteration": -2}, "bilateral: start_iteration must be >= 0 and end_iteration >= 0, or -1 for the end of the run"),
                            ({"levels": 8}, "bilateral: unknown keys ['levels']")):
        with pytest.raises(ValueError) as e:
            trainer_mod.resolve_config({"bilateral": override})
        assert str(e.value) == words


def test_the_three_refusals():
    with pytest.raises(ValueError, match="bilateral: a bilateral grid contains the global affine of exposure.enabled"):
        trainer_mod.resolve_config({"bilateral": {"enabled": True}, "exposure": {"enabled": True}})
    assert trainer_mod.resolve_config({"exposure": {"enabled": True}})["bilateral"]["enabled"] is False
    st = _BilateralStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError) as e:
        _trainer({"n_iterations": 1, "bilateral": {"enabled": True, "grid": [2, 2, 2]}}, stepper=st)
    assert str(e.value) == "bilateral: data-parallel training with bilateral grids is out of scope (the stepper's world_size must be 1)"
    with pytest.raises(ValueError, match="bilateral_gradient: a bilateral grid belongs to ONE view per step"):
        native.NativeTrainStep(None, None, world_size=2, bilateral_gradient=True)
    with pytest.raises(ValueError, match="_FakeStepper leaves no grid gradient"):
        _trainer({"n_iterations": 1, "bilateral": {"enabled": True}}, stepper=_FakeStepper(_model()))
    # composes with the other blocks
    both = trainer_mod.resolve_config({"bilateral": {"enabled": True}, "environment": {"enabled": True}, "pose_refinement": {"enabled": True},
                                       "model": {"background": {"color": "black"}}})
    assert both["bilateral"]["enabled"] and both["environment"]["enabled"]
    for color in ("white", "random"):
        assert trainer_mod.resolve_config({"bilateral": {"enabled": True}, "model": {"background": {"color": color}}})["bilateral"]["enabled"]


def test_flags():
    """The four flags are a table of their own, parsed by main() behind the recorded ones: the default parser and the conf of a
    command line without them are what they were."""
    assert trainer_mod.MAIN_FLAGS == trainer_mod.FLAGS + trainer_mod.ENVIRONMENT_FLAGS + trainer_mod.BILATERAL_FLAGS
    parser = trainer_mod.build_parser(trainer_mod.MAIN_FLAGS)
    conf_of = lambda argv: trainer_mod.config_from_args(parser.parse_args(["--path", "scene"] + argv), trainer_mod.MAIN_FLAGS)
    assert conf_of([])["bilateral"] == {"enabled": False}
    assert trainer_mod.resolve_config(conf_of([]))["bilateral"] == bilateral.DEFAULTS
    assert trainer_mod.resolve_config(conf_of(["--bilateral"]))["bilateral"] == dict(bilateral.DEFAULTS, enabled=True)
    got = trainer_mod.resolve_config(conf_of(["--bilateral", "--bilateral-grid", "8", "6", "4", "--bilateral-lr", "0.01", "--bilateral-tv", "2"]))
    assert got["bilateral"] == dict(bilateral.DEFAULTS, enabled=True, grid=[8, 6, 4], lr=0.01, lambda_tv=2.0)
    assert [f for f, _, _, _ in trainer_mod.BILATERAL_FLAGS] == ["--bilateral", "--bilateral-grid", "--bilateral-lr", "--bilateral-tv"]
    assert "bilateral" not in trainer_mod.config_from_args(trainer_mod.build_parser().parse_args(["--path", "scene"]))
    assert "bilateral" not in trainer_mod.default_config()
    with pytest.raises(SystemExit):
        trainer_mod.build_parser().parse_args(["--path", "scene", "--bilateral"])
    with pytest.raises(ValueError, match="bilateral: a bilateral grid contains the global affine"):
        trainer_mod.resolve_config(conf_of(["--bilateral", "--exposure"]))
    assert "--bilateral [--bilateral-grid X Y L] [--bilateral-lr X] [--bilateral-tv X]" in trainer_mod.__doc__
    assert "--cc-metrics" in dict((f, k["help"]) for f, k, _, _ in trainer_mod.BILATERAL_FLAGS)["--bilateral"]


class _BilateralStepper(_FakeStepper):
    """_FakeStepper with the grid gradient's surface: a batch with a grid leaves a gradient of ones."""
    _bilateral_on = True
    bilateral_gradient = None

    def __init__(self, model, seed=0):
        super().__init__(model, seed)
        self.switches = []

    def enable_bilateral_gradient(self, on):
        self.switches.append(bool(on))

    def step(self, batch):
        grid = getattr(batch, "bilateral_grid", None)
        self.bilateral_gradient = None if grid is None or not self.switches[-1] else torch.ones_like(grid)
        return super().step(batch)


def test_checkpoint_keys_resume_and_the_resume_refusal(tmp_path):
    conf = {"n_iterations": 4, "bilateral": {"enabled": True, "grid": [3, 2, 2], "lr": 0.01, "end_iteration": 3}}
    tr, st, _, _, _ = _trainer(conf, stepper=_BilateralStepper(_model()))
    grids = tr.bilateral
    assert tuple(grids.params.shape) == (3, 12, 2, 2, 3) and grids.lambda_tv == 10.0
    tr.train()
    assert st.switches == [True, True, True, False]                                # the window's switch, step by step
    assert grids.counts.tolist() == [1, 1, 1]                                      # three views, one visit each inside the window
    assert tr.stats["bilateral_grid"] == [3, 2, 2] and tr.stats["bilateral_mean_tv"] == 0.0
    assert abs(tr.stats["bilateral_mean_gain"] - (1.0 - 0.01)) < 1e-6              # one Adam step of size lr from a gradient of ones
    assert torch.equal(tr.bilateral_grids(), grids.params) and not tr.bilateral_grids().is_cuda
    ckpt = tr.checkpoint()
    saved = ckpt["native"]["bilateral"]
    assert set(saved) == {"params", "exp_avg", "exp_avg_sq", "counts"} and all(isinstance(v, torch.Tensor) for v in saved.values())
    path = str(tmp_path / "ckpt.pt")
    torch.save(ckpt, path)
    assert set(torch.load(path, map_location="cpu", weights_only=True)["native"]["bilateral"]) == set(saved)
    # resumed: the same grids and Adam state, and the next step lands on the same bits
    tr2, _, _, _, _ = _trainer(dict(conf, resume=path), stepper=_BilateralStepper(_model()))
    g2 = tr2.bilateral
    for a, b in ((g2.params, grids.params), (g2.m, grids.m), (g2.v, grids.v), (g2.counts, grids.counts)):
        assert torch.equal(a, b)
    grad = torch.randn(grids.params[2].shape, generator=torch.Generator().manual_seed(4))
    for g in (grids, g2):
        g.end(2, grad)
    assert torch.equal(g2.params, grids.params) and not torch.equal(grids.params, saved["params"])
    with pytest.raises(ValueError, match="the checkpoint holds grids of shape"):
        _trainer(dict(conf, resume=path, bilateral=dict(conf["bilateral"], grid=[3, 3, 2])), stepper=_BilateralStepper(_model()))
    with pytest.raises(ValueError, match="bilateral: the checkpoint holds learnt bilateral grids and bilateral.enabled is off; resume with --bilateral"):
        _trainer({"n_iterations": 4, "resume": path}, stepper=_BilateralStepper(_model()))
    # without grids: no key, no object
    tr3, _, _, _, _ = _trainer({"n_iterations": 1})
    assert "bilateral" not in tr3.checkpoint()["native"] and tr3.bilateral is None and tr3.bilateral_grids() is None


def test_bindings():
    lib = _capi.load()
    assert lib.gut_abi_version() == 6 == _capi.GUT_ABI_VERSION
    for name in ("gut_bilateral_workspace_bytes", "gut_bilateral_slice", "gut_bilateral_backward", "gut_bilateral_backward_image",
                 "gut_bilateral_adam_step"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    grid_p = C.POINTER(_capi.GutBilateralGrid)
    assert lib.gut_bilateral_slice.argtypes == [vp, i32, i32, vp, vp, f32, grid_p, vp]
    assert lib.gut_bilateral_backward.argtypes == [vp, i32, i32, vp, vp, f32, grid_p, vp, f32, vp, vp, vp]
    assert lib.gut_bilateral_backward_image.argtypes == [vp, i32, i32, vp, vp, f32, grid_p, vp, vp]
    assert lib.gut_bilateral_adam_step.argtypes == [vp, vp, vp, vp, vp, vp, C.c_int64, f32, f32, f32, f32]
    assert lib.gut_bilateral_workspace_bytes.argtypes == [i32, i32, i32] and lib.gut_bilateral_workspace_bytes.restype is C.c_size_t
    assert lib.gut_exposure_adam_step.argtypes == [vp, vp, vp, vp, vp, vp, f32, f32, f32, f32]         # the exposure's keeps its signature
    assert C.sizeof(_capi.GutBilateralGrid) == 24
    assert lib.gut_bilateral_workspace_bytes(8, 16, 16) == 8 * 12 * 8 * 16 * 16 + 16
    for bad in ((0, 16, 16), (8, 0, 16), (8, 16, 257), (-1, 1, 1)):
        assert lib.gut_bilateral_workspace_bytes(*bad) == 0
    assert 12 * _capi.BILATERAL_MAX_DIM ** 3 < 2 ** 32 and _capi.BILATERAL_MAX_DIM == bilateral.MAX_DIM
    assert 3 * 3 * 8 * 12 <= _capi.BILATERAL_TABLE                                 # the shipped grid's footprint fits the table
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gut_hip.h")).read()
    assert "#define GUT_BILATERAL_MAX_DIM 256" in header and "#define GUT_BILATERAL_TABLE 1024" in header
    assert "#define GUT_ABI_VERSION 6" in header and "gut_bilateral_adam_step" in header.split("#define GUT_ABI_VERSION 6")[0]


def test_error_returns_are_host_side():
    """Every refusal is decided before anything is queued, so it is the same without a GPU: nothing here launches."""
    lib = _capi.load()
    buf = np.zeros((64,), np.float32)
    some = (buf.ctypes.data + 15) & ~15        # 16-byte aligned; never dereferenced: every call below is refused on the host
    grid = lambda ptr=some, L=2, Gh=3, Gw=4: C.byref(_capi.GutBilateralGrid(ptr, L, Gh, Gw))

    def refused(rc, words):
        assert rc != 0 and words in lib.gut_last_error().decode(), lib.gut_last_error()
    sl = lib.gut_bilateral_slice
    refused(sl(None, 4, 4, some, None, 0.0, None, some), "gut_bilateral_slice: null grid")
    refused(sl(None, 4, 4, some, None, 0.0, grid(None), some), "null d_grid")
    refused(sl(None, 4, 4, None, None, 0.0, grid(), some), "null d_rgba")
    refused(sl(None, 4, 4, some, None, 0.0, grid(), None), "null d_rgba_out")
    refused(sl(None, 4, 4, some, None, 0.0, grid(L=0), some), "grid dimensions must be 1 .. 256, got 0 x 3 x 4")
    refused(sl(None, 4, 4, some, None, 0.0, grid(Gh=257), some), "grid dimensions must be 1 .. 256, got 2 x 257 x 4")
    refused(sl(None, 4, 4, some, None, 0.0, grid(Gw=-1), some), "grid dimensions must be 1 .. 256")
    refused(sl(None, 0, 4, some, None, 0.0, grid(), some), "an empty image")
    refused(sl(None, 4, 0, some, None, 0.0, grid(), some), "an empty image")
    refused(sl(None, 1 << 15, (1 << 15) + 1, some, None, 0.0, grid(), some), "exceeds 2^30 pixels")
    refused(sl(None, 4, 4, some + 4, None, 0.0, grid(), some), "d_rgba is not 16-byte aligned")
    bw = lib.gut_bilateral_backward
    refused(bw(None, 4, 4, some, None, 0.0, None, some, 0.0, some, some, some), "gut_bilateral_backward: null grid")
    refused(bw(None, 4, 4, None, None, 0.0, grid(), some, 0.0, some, some, some), "null d_rgba")
    for k in range(4):
        ptrs = [some, some, some, some]
        ptrs[k] = None
        refused(bw(None, 4, 4, some, None, 0.0, grid(), ptrs[0], 0.0, ptrs[1], ptrs[2], ptrs[3]),
                "null d_rgba_out_grad, d_workspace, d_rgba_grad or d_grid_grad")
    refused(bw(None, 4, 4, some, None, 0.0, grid(L=300), some, 0.0, some, some, some), "grid dimensions must be 1 .. 256")
    refused(bw(None, 0, 0, some, None, 0.0, grid(), some, 0.0, some, some, some), "an empty image")
    refused(bw(None, 1 << 16, 1 << 15, some, None, 0.0, grid(), some, 0.0, some, some, some), "exceeds 2^30 pixels")
    for tv in (float("nan"), float("inf"), float("-inf")):
        refused(bw(None, 4, 4, some, None, 0.0, grid(), some, tv, some, some, some), "lambda_tv must be finite")
    refused(bw(None, 4, 4, some, None, 0.0, grid(), some, 0.0, some + 4, some, some), "d_workspace is not 8-byte aligned")
    bi = lib.gut_bilateral_backward_image
    refused(bi(None, 4, 4, some, None, 0.0, None, some, some), "gut_bilateral_backward_image: null grid")
    refused(bi(None, 4, 4, None, None, 0.0, grid(), some, some), "null d_rgba")
    refused(bi(None, 4, 4, some, None, 0.0, grid(), None, some), "null d_rgba_out_grad or d_rgba_grad")
    refused(bi(None, 4, 4, some, None, 0.0, grid(), some, None), "null d_rgba_out_grad or d_rgba_grad")
    refused(bi(None, 4, 4, some, None, 0.0, grid(Gw=0), some, some), "grid dimensions must be 1 .. 256")
    refused(bi(None, 4, 0, some, None, 0.0, grid(), some, some), "an empty image")
    refused(bi(None, 4, 4, some, None, 0.0, grid(), some, some + 8), "not 16-byte aligned")
    ad = lib.gut_bilateral_adam_step
    for k in range(5):
        ptrs = [some] * 5
        ptrs[k] = None
        refused(ad(None, *ptrs, 12, 0.01, 0.9, 0.999, 1e-15), "gut_bilateral_adam_step: null pointer argument")
    refused(ad(None, some, some, some, some, some, 0, 0.01, 0.9, 0.999, 1e-15), "n must be 1 ..")
    refused(ad(None, some, some, some, some, some, 12 * 256 ** 3 + 1, 0.01, 0.9, 0.999, 1e-15), "n must be 1 ..")
