"""`model.background.color: random` without a GPU: the Trainer takes the reference's three colours and refuses others with the
reference's wording (model/background.py:66-70), the CLI likewise, a checkpoint of a `random` run stores the zero colour
BackgroundColor.setup keeps for it, the model remembers its last draw, and the fused loss' background argument is normalised to one
contiguous float32 [H,W,3] plane whatever form it came in."""
import importlib

import pytest
import torch

from tests.test_cpu_trainer import _FakeStepper, _batch, _model, _trainer

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
losses = importlib.import_module("3dgrut_amd.losses")
native = importlib.import_module("3dgrut_amd.native")


def _conf(color):
    return dict(n_iterations=2, val_frequency=1000, model=dict(background=dict(color=color)))


@pytest.mark.parametrize("color", ["black", "white", "random"])
def test_the_trainer_takes_the_three_colours(color):
    c = trainer_mod.resolve_config(_conf(color))
    assert c["model"]["background"] == {"name": "background-color", "color": color}
    assert trainer_mod.check_background_color(c) == color
    tr, st, _, _, _ = _trainer(_conf(color))
    assert tr.conf["model"]["background"]["color"] == color
    tr.train()
    assert len(st.steps) == 2


def test_the_default_colour_is_black():
    assert trainer_mod.resolve_config({})["model"]["background"]["color"] == "black"


@pytest.mark.parametrize("color", ["green", "", "Random", None, 1.0])
def test_the_trainer_refuses_other_colours(color):
    with pytest.raises(ValueError, match="Background color must be one of 'white', 'black', 'random'"):
        _trainer(_conf(color))


def test_cli_background_option():
    ap = trainer_mod.build_parser()
    assert ap.parse_args(["--path", "x"]).background is None
    for color in ("black", "white", "random"):
        assert ap.parse_args(["--path", "x", "--background", color]).background == color
    for bad in ("green", "Random", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(["--path", "x", "--background", bad])


@pytest.mark.parametrize("color,value", [("random", 0.0), ("black", 0.0), ("white", 1.0)])
def test_checkpoint_colour(color, value):
    tr, _, _, _, _ = _trainer(_conf(color))
    ck = tr.checkpoint()
    assert torch.equal(ck["background"]["color"], torch.full((3,), value)) and ck["background"]["color"].dtype == torch.float32
    assert ck["config"]["model"]["background"]["color"] == color


def test_the_model_keeps_its_last_draw():
    m = native.NativeGaussianModel.from_tensors(torch.zeros((2, 12)), torch.zeros((2, 48)), background_color="random")
    assert m.last_background is None
    rays = torch.zeros((1, 5, 7, 3))
    rgb, opacity = torch.full((1, 5, 7, 3), 0.25), torch.full((1, 5, 7, 1), 0.5)
    out, _ = m.background(None, rays, rgb, opacity, train=False)           # not training: black, nothing drawn
    assert torch.equal(out, rgb) and m.last_background is None
    torch.manual_seed(4)
    out, _ = m.background(None, rays, rgb, opacity, train=True)
    torch.manual_seed(4)
    expected = torch.rand_like(rays)                                        # the reference's draw (background.py:86)
    assert tuple(m.last_background.shape) == (5, 7, 3) and torch.equal(m.last_background, expected[0])
    assert torch.equal(out, rgb + expected * (1.0 - opacity))
    torch.manual_seed(4)
    assert torch.equal(m.draw_background(rays), expected[0])                # what the fused branch calls: the same draw


def test_background_argument_normalisation():
    H, W = 5, 7
    b = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(1))
    for form in (b, b[None], b.double(), b.half().float()[None], b.transpose(0, 1).contiguous().transpose(0, 1)):
        p = losses._plane_background(form, H, W, "cpu")
        assert p.dtype == torch.float32 and tuple(p.shape) == (H, W, 3) and p.is_contiguous()
        assert torch.equal(p, form.reshape(H, W, 3).float())
    assert losses._plane_background(b, H, W, "cpu").data_ptr() == b.data_ptr()          # already in form: a view, no copy
    colour = torch.tensor([0.25, 0.5, 0.875], dtype=torch.float64)
    p = losses._plane_background(colour, H, W, "cpu")
    assert p.dtype == torch.float32 and tuple(p.shape) == (H, W, 3) and p.is_contiguous()
    assert torch.equal(p, colour.float().expand(H, W, 3))
    as_int = losses._plane_background(torch.ones((H, W, 3), dtype=torch.uint8), H, W, "cpu")
    assert as_int.dtype == torch.float32 and bool((as_int == 1.0).all())
    for bad in (b[..., 0], torch.zeros((H, W, 4)), torch.zeros((2, H, W, 3)), torch.zeros((W, H, 3)), torch.zeros((1, 3)), torch.zeros((4,))):
        with pytest.raises(ValueError, match="background"):
            losses._plane_background(bad, H, W, "cpu")


def test_a_string_background_other_than_black_or_white_is_still_refused():
    z = torch.zeros((12, 12, 4))
    with pytest.raises(ValueError, match="background"):
        losses.fused_photometric_loss(z, z[..., :3], "random")
