"""`model.background.color: random` through the train step and the trainer: the fused loss sees the very colours the torch branch
draws (one torch.rand_like(rays_dir) per step, kept as model.last_background), one step moves the parameters as the torch branch's
does, with and without a mask, and a short run lands where the torch branch's run lands."""
import importlib

import pytest
import torch

from tests.common import cams, make_view, rel_l2, scenes, to_batch
from tests.synthetic_colmap import load_scene, write_synthetic_colmap

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
native = importlib.import_module("3dgrut_amd.native")
losses = importlib.import_module("3dgrut_amd.losses")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
schedule_mod = importlib.import_module("3dgrut_amd.schedule")
evaluate = importlib.import_module("3dgrut_amd.evaluate").evaluate
DEV = "cuda:0"
H, W = 64, 96
BLOCKS = (("positions", slice(0, 3)), ("density", slice(3, 4)), ("rotation", slice(4, 8)), ("scale", slice(8, 11)))


def _one_step(sc, batch, fused_loss):
    """One step of a fresh NativeTrainStep with a random background under torch.manual_seed(0); the rgba its loss saw is kept."""
    model = native.NativeGaussianModel(sc, device=DEV, background_color="random")
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fused_loss=fused_loss)   # no regulariser, zero moments
    assert model.last_background is None
    raw0, feat0 = model.raw.clone(), model.features.clone()
    seen, inner = [], st._loss
    st._loss = lambda b, rgba: (seen.append(rgba.clone()), inner(b, rgba))[1]
    torch.manual_seed(0)
    loss, out = st.step(batch)
    torch.cuda.synchronize()
    return st, raw0, feat0, loss, out, seen[0]


def _batch(masked):
    # the view of tests/test_gpu_masked_training.py: both image halves hold plenty of Gaussians
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.25, -0.1, -3.5), (0.25, 0.0, 0.0)), fx=110.0)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    if masked:
        mask = torch.ones((1, H, W, 1), dtype=torch.float32)
        mask[:, :, :W // 2] = 0.0
        batch.mask = mask.to(DEV)
    return batch


@pytest.mark.parametrize("masked", [False, True])
def test_one_step_with_a_random_background(masked):
    """The fused branch and the torch branch of one step on a 64x96 view, each after torch.manual_seed(0): the same draw, the fused
    step's loss is the background-plane loss of its own render over that draw, the two losses agree to 1e-5 and every parameter
    block to rel-L2 2e-5 (the one-step bounds of tests/test_gpu_masked_training.py); with the left half masked out, the Gaussians
    wholly in it keep their bits — the alpha gradient included."""
    sc = scenes.scene_c1(4000, 21)
    batch = _batch(masked)
    mask = getattr(batch, "mask", None)
    st, raw0, feat0, loss, out, rgba = _one_step(sc, batch, fused_loss=True)
    B = st.model.last_background
    assert tuple(B.shape) == (H, W, 3) and B.dtype == torch.float32 and float(B.min()) >= 0.0 and float(B.max()) < 1.0
    assert float(B.std()) > 0.25                                                       # uniform per pixel, not one colour
    loss3, rgba_grad = losses.fused_photometric_loss(rgba, batch.rgb_gt, B, 0.8, 0.2, mask=mask)
    assert float(loss) == float(loss3[0])
    assert float(rgba_grad[..., 3].abs().max()) > 0
    black3, _ = losses.fused_photometric_loss(rgba, batch.rgb_gt, "black", 0.8, 0.2, mask=mask)
    assert abs(float(black3[0]) - float(loss)) > 1e-3                                  # (the background does show through this render)
    assert torch.equal(out["pred_rgb"][0], rgba[..., :3] + B * (1.0 - rgba[..., 3:]))  # unmasked, over the same draw

    tt, traw0, tfeat0, tloss, tout, trgba = _one_step(sc, batch, fused_loss=False)
    assert torch.equal(traw0, raw0) and torch.equal(tfeat0, feat0)
    assert torch.equal(tt.model.last_background, B)
    print(f"\n[random background step, masked={masked}] loss fused {float(loss):.8f} torch {float(tloss):.8f}")
    assert abs(float(tloss) - float(loss)) <= 1e-5
    keep = torch.ones(st.model.num_gaussians, dtype=torch.bool, device=DEV)
    if masked:
        n = st.model.num_gaussians
        cnt = st.raster.debug_buffer("tiles_count")
        pos = st.raster.debug_buffer("proj_pos").view(n, 2)
        ext = st.raster.debug_buffer("extent").view(n, 2)
        hidden = (cnt > 0) & (pos[:, 0] + ext[:, 0] + 16.0 <= W // 2)    # every tile it lies in is left of the x = 48 tile border
        assert int(hidden.sum()) >= 0.1 * n
        for s in (st, tt):
            assert torch.equal(s.model.raw[hidden], raw0[hidden]) and torch.equal(s.model.features[hidden], feat0[hidden])
        keep = ~hidden
    assert not torch.equal(st.model.raw[keep], raw0[keep])
    rest = keep.cpu().numpy()
    a, b = st.model.raw.cpu().numpy()[rest], tt.model.raw.cpu().numpy()[rest]
    for name, cols in BLOCKS:
        assert rel_l2(a[:, cols], b[:, cols]) <= 2e-5, name
    assert rel_l2(st.model.features.cpu().numpy()[rest], tt.model.features.cpu().numpy()[rest]) <= 2e-5


# ---- a short run ----
NO_EVENTS = dict(densify=dict(start_iteration=-1, end_iteration=-1), prune=dict(start_iteration=-1, end_iteration=-1),
                 reset_density=dict(start_iteration=-1, end_iteration=-1))
PSNR_TOL = 0.3          # tests/test_gpu_trainer.py's tolerance; its measured repeat-to-repeat spread is below 0.1 dB


def _torch_branch_stepper(conf, init, extent):
    """The NativeTrainStep Trainer builds for `conf` (the reference's default rates, which are NativeTrainStep's own), with the loss
    in image-sized torch autograd."""
    c = trainer_mod.resolve_config(conf)
    prog, sp = c["model"]["progressive_training"], c["scheduler"]["positions"]
    sched = schedule_mod.TrainSchedule(extent, lr_init=float(c["optimizer"]["params"]["positions"]["lr"]), lr_final=float(sp["lr_final"]),
                                       max_steps=int(sp["max_steps"]), init_n_features=int(prog["init_n_features"]),
                                       max_n_features=int(prog["max_n_features"]), increase_frequency=int(prog["increase_frequency"]),
                                       increase_step=int(prog["increase_step"]))
    model = native.NativeGaussianModel(init, sh_degree=sched.n_active_features, background_color=c["model"]["background"]["color"],
                                       spatial_order=True)
    return native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=extent, eps=float(c["optimizer"]["eps"]), schedule=sched,
                                  fused_loss=False, **losses.loss_weights(c["loss"]))


def test_a_short_run_lands_where_the_torch_branch_lands(tmp_path):
    """300 steps on a reduced synthetic COLMAP scene (16 views of 200 x 200, every 8th held out, no densification) with
    model.background.color: random, once with the Trainer's own stepper (the fused loss over the drawn plane) and once with a
    NativeTrainStep(fused_loss=False): held-out PSNR within the trainer tests' 0.3 dB of each other, both above the initial
    model's.  The yardstick is the torch branch's run; no value measured on the fused branch is written here."""
    root = write_synthetic_colmap(str(tmp_path / "scene"), n_views=16, size=200, n_teacher=50_000, n_points=5_000)
    init, tb, vb, extent = load_scene(root)
    conf = dict(n_iterations=300, val_frequency=10 ** 9, test_last=False, out_dir="", seed=0, model=dict(background=dict(color="random")),
                strategy=dict(method="GSStrategy", **NO_EVENTS))
    psnr = []
    for fused in (True, False):
        torch.manual_seed(0)
        stepper = None if fused else _torch_branch_stepper(conf, init, extent)
        tr = trainer_mod.Trainer(conf, init, tb, test_batches=vb, scene_extent=extent, stepper=stepper)
        assert tr.model.background_color == "random" and tr.stepper.fused_loss == fused
        initial = evaluate(tr.model, tr.tracer, vb)["mean_psnr"]             # the untrained initial model
        if fused:
            psnr.append(initial)
        tr.train()
        assert tuple(tr.model.last_background.shape) == (200, 200, 3)
        psnr.append(evaluate(tr.model, tr.tracer, vb)["mean_psnr"])
        del tr, stepper
        torch.cuda.empty_cache()
    p0, p_fused, p_torch = psnr
    print(f"\n[random background run] held-out psnr: initial {p0:.3f}, fused loss {p_fused:.3f}, torch branch {p_torch:.3f}")
    assert p_fused > p0 and p_torch > p0
    assert abs(p_fused - p_torch) <= PSNR_TOL
