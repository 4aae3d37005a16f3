"""Masked views through the train step and the trainer: what a mask hides moves nothing (NativeTrainStep, both loss branches), and a
run on views with masked-out distractors, read through the COLMAP reader's `_mask.png` files, lands where the run on clean views does
while the same run without the masks does not."""
import dataclasses
import importlib
import os
import shutil

import numpy as np
import pytest
import torch

from tests.common import cams, make_view, rel_l2, scenes, to_batch
from tests.synthetic_colmap import load_scene, write_synthetic_colmap

pytestmark = pytest.mark.gpu
gut = importlib.import_module("3dgrut_amd")
native = importlib.import_module("3dgrut_amd.native")
losses = importlib.import_module("3dgrut_amd.losses")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
evaluate = importlib.import_module("3dgrut_amd.evaluate").evaluate
DEV = "cuda:0"


def _one_step(sc, batch, fused_loss):
    model = native.NativeGaussianModel(sc, device=DEV)
    st = native.NativeTrainStep(model, gut.Tracer({"render": {}}), scene_extent=1.0, fused_loss=fused_loss)   # no regulariser, zero moments
    assert not st.m12.any() and not st.v48.any()
    raw0, feat0 = model.raw.clone(), model.features.clone()
    loss, out = st.step(batch)
    torch.cuda.synchronize()
    return st, raw0, feat0, loss, out


def test_masked_pixels_move_nothing():
    """One step of a fresh NativeTrainStep (zero moments: Adam with a zero gradient moves nothing) on a 64x96 view whose left half is
    masked out: every Gaussian whose projected extent, plus a 16-pixel tile of margin, lies in the masked half keeps its raw and
    feature rows bit for bit — with the fused loss and with the torch branch — and the two branches agree on every other row to the
    one-step tolerance of tests/test_gpu_native.py (rel-L2 2e-5 per block, loss 1e-5).  Fails where the mask is ignored."""
    H, W = 64, 96
    sc = scenes.scene_c1(4000, 21)
    # the camera stands right of the cloud's centre line, so the cloud sits left of the image's: both halves hold plenty of Gaussians
    view = make_view("pinhole", W, H, cams.look_at_c2w((0.25, -0.1, -3.5), (0.25, 0.0, 0.0)), fx=110.0)
    batch = to_batch(view, DEV)
    batch.rgb_gt = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    mask = torch.ones((1, H, W, 1), dtype=torch.float32)
    mask[:, :, :W // 2] = 0.0
    batch.mask = mask.to(DEV)

    st, raw0, feat0, loss, out = _one_step(sc, batch, fused_loss=True)
    n = st.model.num_gaussians
    # the forward's projected centres and extents, in pixels, one row per Gaussian (this library's names for the buffers)
    cnt = st.raster.debug_buffer("tiles_count")
    pos = st.raster.debug_buffer("proj_pos").view(n, 2)
    ext = st.raster.debug_buffer("extent").view(n, 2)
    visible = cnt > 0
    hidden = visible & (pos[:, 0] + ext[:, 0] + 16.0 <= W // 2)          # every tile it lies in is left of the x = 48 tile border
    shown = visible & (pos[:, 0] > W // 2)
    print(f"\n[masked step] {int(visible.sum())} of {n} Gaussians visible, {int(hidden.sum())} wholly in the masked half, "
          f"{int(shown.sum())} centred in the other half")
    assert int(hidden.sum()) >= 0.1 * n and int(shown.sum()) >= 0.1 * n
    assert torch.equal(st.model.raw[hidden], raw0[hidden]) and torch.equal(st.model.features[hidden], feat0[hidden])
    assert not torch.equal(st.model.raw[shown], raw0[shown]) and not torch.equal(st.model.features[shown], feat0[shown])
    # the loss returned is the masked loss of the step's own render, and the render returned is not masked
    pred = out["pred_rgb"][0]
    rgba = torch.cat([pred, torch.zeros_like(pred[..., :1])], dim=-1).contiguous()   # black background: alpha is not read
    loss3, rgba_grad = losses.fused_photometric_loss(rgba, batch.rgb_gt, "black", 0.8, 0.2, mask=batch.mask)
    assert float(loss) == float(loss3[0])
    assert bool((rgba_grad[:, :W // 2] == 0.0).all()) and float(rgba_grad[:, W // 2:].abs().max()) > 0
    plain3, _ = losses.fused_photometric_loss(rgba, batch.rgb_gt, "black", 0.8, 0.2)
    assert abs(float(plain3[0]) - float(loss)) > 1e-3
    assert float(pred[:, :W // 2].abs().max()) > 0

    # the torch branch (what a random background or a non-contiguous gt takes)
    tt, traw0, tfeat0, tloss, _ = _one_step(sc, batch, fused_loss=False)
    assert torch.equal(traw0, raw0) and torch.equal(tfeat0, feat0)
    assert abs(float(tloss) - float(loss)) <= 1e-5
    assert torch.equal(tt.model.raw[hidden], raw0[hidden]) and torch.equal(tt.model.features[hidden], feat0[hidden])
    rest = (~hidden).cpu().numpy()
    a, b = st.model.raw.cpu().numpy()[rest], tt.model.raw.cpu().numpy()[rest]
    for name, cols in (("positions", slice(0, 3)), ("density", slice(3, 4)), ("rotation", slice(4, 8)), ("scale", slice(8, 11))):
        assert rel_l2(a[:, cols], b[:, cols]) <= 2e-5, name
    assert rel_l2(st.model.features.cpu().numpy()[rest], tt.model.features.cpu().numpy()[rest]) <= 2e-5


# ---- distractors ----
NO_EVENTS = dict(densify=dict(start_iteration=-1, end_iteration=-1), prune=dict(start_iteration=-1, end_iteration=-1),
                 reset_density=dict(start_iteration=-1, end_iteration=-1))
SQUARE = 120            # 9 % of a 400 x 400 view
PSNR_TOL = 0.3          # tests/test_gpu_trainer.py's tolerance; its measured repeat-to-repeat spread is below 0.1 dB
# held-out PSNR (dB) of the three runs below, measured once on an MI355X
MEASURED_CLEAN, MEASURED_MASKED, MEASURED_UNMASKED = 21.227, 21.084, 20.527


def write_distractors(clean_dir, root, test_split_interval=8):
    """A copy of the synthetic COLMAP folder in which every TRAINING image carries a 120 x 120 square of (1, 0, 1) at a position that
    moves with the view index, and a `_mask.png` next to it that is 0 on the square and 255 elsewhere.  Held-out images stay clean."""
    from PIL import Image
    shutil.copytree(clean_dir, root)
    names = sorted(os.listdir(os.path.join(root, "images")))
    n_train = 0
    for i, name in enumerate(names):
        if i % test_split_interval == 0:
            continue
        path = os.path.join(root, "images", name)
        with Image.open(path) as f:
            img = np.asarray(f.convert("RGB")).copy()
        h, w = img.shape[:2]
        x0, y0 = (37 * i) % (w - SQUARE), (53 * i) % (h - SQUARE)
        img[y0:y0 + SQUARE, x0:x0 + SQUARE] = (255, 0, 255)
        Image.fromarray(img).save(path)
        m = np.full((h, w), 255, np.uint8)
        m[y0:y0 + SQUARE, x0:x0 + SQUARE] = 0
        Image.fromarray(m).save(os.path.splitext(path)[0] + "_mask.png")
        n_train += 1
    return n_train


def three_runs(clean_dir, corrupted_dir):
    """Held-out PSNR on the CLEAN test views after 1 000 steps (same init, seed and view order, no densification) on: the clean
    views; the views with distractors and their masks, as the reader hands them over; the same views with the masks taken off."""
    init, tb, vb, extent = load_scene(clean_dir)
    n_train = write_distractors(clean_dir, corrupted_dir)
    init_c, tb_masked, vb_c, extent_c = load_scene(corrupted_dir)
    assert n_train == len(tb_masked) == len(tb) and extent_c == extent
    assert all(b.mask is not None and tuple(b.mask.shape) == (1, 400, 400, 1) for b in tb_masked) and all(b.mask is None for b in vb_c)
    hidden = float(torch.stack([1.0 - b.mask.mean() for b in tb_masked]).mean())
    assert abs(hidden - SQUARE * SQUARE / 160000.0) < 1e-5
    assert all(torch.equal(a.rgb_gt, b.rgb_gt) for a, b in zip(vb, vb_c))                        # held-out views: untouched
    assert all(torch.equal((a.rgb_gt * b.mask), (b.rgb_gt * b.mask)) for a, b in zip(tb, tb_masked))   # outside the square: untouched
    tb_unmasked = [dataclasses.replace(b, mask=None) for b in tb_masked]
    conf = dict(n_iterations=1000, val_frequency=10 ** 9, test_last=False, out_dir="", seed=0, strategy=dict(method="GSStrategy", **NO_EVENTS))
    psnr = []
    for batches in (tb, tb_masked, tb_unmasked):
        tr = trainer_mod.Trainer(conf, init, batches, test_batches=vb, scene_extent=extent)
        tr.train()
        psnr.append(evaluate(tr.model, tr.tracer, vb)["mean_psnr"])
        del tr
        torch.cuda.empty_cache()
    return psnr


def test_masked_distractors_train_like_clean_views(tmp_path):
    """Three 1 000-step runs on the synthetic COLMAP scene (32 views of 400 x 400, every 8th held out), scored on the clean held-out
    views: A on clean views, B on views with a 120 x 120 magenta square each (9 % of the view) and the `_mask.png` files that hide
    it, loaded through ColmapScene, C on the same views without the masks.  Measured on MI355X: A 21.227 dB, B 21.084 dB, C 20.527 dB
    (A - B = 0.14 dB, B - C = 0.56 dB).  B must stay within the measured A - B plus the trainer tests' 0.3 dB of A, and keep at least
    half of the measured lead over C."""
    clean = write_synthetic_colmap(str(tmp_path / "clean"))
    a, b, c = three_runs(clean, str(tmp_path / "corrupted"))
    print(f"\n[distractors] held-out psnr: clean {a:.3f}, masked {b:.3f}, distractors without masks {c:.3f}")
    assert b >= a - ((MEASURED_CLEAN - MEASURED_MASKED) + PSNR_TOL)
    assert b - c >= 0.5 * (MEASURED_MASKED - MEASURED_UNMASKED)
