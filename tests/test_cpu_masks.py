"""Masked views without a GPU: the COLMAP reader's `<image stem>_mask.png` files (threshold, shape, the down-sampled images folder,
a missing file, a wrong size) and who may be handed a masked batch (the Trainer asks the stepper; evaluation takes and ignores masks)."""
import importlib
import os

import numpy as np
import pytest
import torch


io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
trainer_mod = importlib.import_module("3dgrut_amd.trainer")
evaluate_mod = importlib.import_module("3dgrut_amd.evaluate")
Batch = importlib.import_module("3dgrut_amd.protocols").Batch

W, H = 24, 16
NAMES = ("a.png", "b.jpg", "sub/c.png")


def _colmap_dir(root):
    """sparse/0 with one 24x16 PINHOLE camera and three images; images/ and images_2/ hold grey PNG / JPEG files of the right sizes."""
    from PIL import Image
    cam = io_colmap.ColmapCamera(1, "PINHOLE", W, H, np.array([20.0, 20.0, W / 2, H / 2], np.float64))
    images = [io_colmap.ColmapImage(i + 1, np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1 * i, 0.0, 2.0]), 1, n) for i, n in enumerate(NAMES)]
    io_colmap.write_model_binary(os.path.join(root, "sparse", "0"), {1: cam}, images, np.zeros((4, 3)), np.zeros((4, 3), np.uint8))
    for folder, (w, h) in (("images", (W, H)), ("images_2", (W // 2, H // 2))):
        for n in NAMES:
            path = os.path.join(root, folder, n)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(path)
    return root


def _write_mask(root, folder, name, values):
    from PIL import Image
    path = os.path.join(root, folder, os.path.splitext(name)[0] + "_mask.png")
    Image.fromarray(values).save(path)
    return path


def test_reader_thresholds_and_shapes_the_mask(tmp_path):
    root = _colmap_dir(str(tmp_path))
    values = np.zeros((H, W), np.uint8)
    values[:, 6:12], values[:, 12:18], values[:, 18:] = 127, 128, 255
    _write_mask(root, "images", "a.png", values)
    # a colour mask file goes through convert("L") like any other: white on black
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[4:, :] = 255
    _write_mask(root, "images", "sub/c.png", rgb)
    scene = io_colmap.ColmapScene(root, "train", 1, test_split_interval=0)
    assert [im.name for im in scene.images] == list(NAMES)
    m = scene.load_mask(0)
    assert m.shape == (1, H, W, 1) and m.dtype == np.float32
    assert np.array_equal(m[0, :, :, 0], np.repeat(np.array([0, 0, 1, 1], np.float32), 6)[None, :].repeat(H, 0))
    b = scene.batch(0, device="cpu")
    assert b.mask.dtype == torch.float32 and tuple(b.mask.shape) == (1, H, W, 1) and tuple(b.rgb_gt.shape) == (1, H, W, 3)
    assert torch.equal(b.mask, torch.as_tensor(m))
    assert scene.load_mask(1) is None and scene.batch(1, device="cpu").mask is None       # b_mask.png does not exist
    c = scene.batch(2, device="cpu").mask
    assert float(c[0, :4].max()) == 0.0 and float(c[0, 4:].min()) == 1.0


def test_reader_takes_the_mask_from_the_downsampled_folder(tmp_path):
    root = _colmap_dir(str(tmp_path))
    _write_mask(root, "images", "b.jpg", np.full((H, W), 255, np.uint8))                    # full size: not the one to read
    half = np.full((H // 2, W // 2), 255, np.uint8)
    half[:, :5] = 0
    _write_mask(root, "images_2", "b.jpg", half)
    scene = io_colmap.ColmapScene(root, "train", 2, test_split_interval=0)
    b = scene.batch(1, device="cpu")
    assert tuple(b.mask.shape) == (1, H // 2, W // 2, 1) and tuple(b.rgb_gt.shape) == (1, H // 2, W // 2, 3)
    assert torch.equal(b.mask[0, :, :, 0], torch.as_tensor(half > 0).float())
    assert scene.batch(0, device="cpu").mask is None


def test_reader_refuses_a_mask_of_another_size(tmp_path):
    root = _colmap_dir(str(tmp_path))
    _write_mask(root, "images", "a.png", np.full((H, W - 1), 255, np.uint8))
    scene = io_colmap.ColmapScene(root, "train", 1, test_split_interval=0)
    with pytest.raises(ValueError, match="mask"):
        scene.load_mask(0)
    with pytest.raises(ValueError, match="mask"):
        scene.batch(0, device="cpu")
    # without the image file the camera's (down-sampled) resolution is the size to have
    os.remove(os.path.join(root, "images", "a.png"))
    with pytest.raises(ValueError, match="mask"):
        scene.load_mask(0)
    _write_mask(root, "images", "a.png", np.full((H, W), 255, np.uint8))
    assert scene.load_mask(0).shape == (1, H, W, 1) and scene.batch(0, device="cpu").rgb_gt is None


def _batch(tag, mask=False, gt=True):
    z = torch.zeros((1, 12, 12, 3))
    b = Batch(rays_ori=z, rays_dir=z, T_to_world=torch.eye(4)[None], rgb_gt=z.clone() if gt else None,
              mask=torch.ones((1, 12, 12, 1)) if mask else None)
    b.tag = tag
    return b


class _Model:
    num_gaussians = 5
    raw = torch.zeros((5, 12))


class _FakeStepper:
    """What Trainer.train() uses of a stepper, nothing else: step() records the view and the mask it was handed."""

    def __init__(self):
        self.model, self.lr12, self.steps, self.masks = _Model(), np.full(12, 1e-3, np.float32), [], []

    def step(self, batch):
        self.steps.append(batch.tag)
        self.masks.append(batch.mask)
        return torch.tensor(0.25), {}


class _MaskAwareStepper(_FakeStepper):
    supports_masks = True


class _FakeStrategy:
    def post_optimizer_step(self, step, arg):
        pass


class _FakeEvaluator:
    def __init__(self):
        self.steps = []

    def __call__(self, model, tracer, batches, out_dir, step):
        self.steps.append(step)
        return dict(mean_psnr=20.0, mean_ssim=0.5)


def test_trainer_hands_masked_training_batches_to_a_stepper_that_supports_them():
    st = _MaskAwareStepper()
    batches = [_batch(0), _batch(1, mask=True)]
    tr = trainer_mod.Trainer(dict(n_iterations=4, val_frequency=1000, checkpoint=dict(iterations=[])), None, batches, stepper=st,
                             strategy=_FakeStrategy(), evaluator=_FakeEvaluator())
    tr.train()
    assert sorted(st.steps) == [0, 0, 1, 1]
    for view, mask in zip(st.steps, st.masks):                                         # the mask reaches step() with its batch
        assert (mask is not None) == (view == 1)


def test_trainer_takes_masked_validation_and_test_batches_with_any_stepper():
    st = _FakeStepper()
    assert not hasattr(st, "supports_masks")
    ev = _FakeEvaluator()
    tr = trainer_mod.Trainer(dict(n_iterations=2, val_frequency=1, checkpoint=dict(iterations=[])), None, [_batch(0)],
                             val_batches=[_batch(100, mask=True)], test_batches=[_batch(200, mask=True)], stepper=st,
                             strategy=_FakeStrategy(), evaluator=ev)
    tr.train()
    assert ev.steps == [1]
    # ... and the same stepper is still refused a masked TRAINING batch, in words that name the mask
    with pytest.raises(ValueError, match="mask"):
        trainer_mod.Trainer({}, None, [_batch(0, mask=True)], stepper=st, strategy=_FakeStrategy())


def test_evaluation_accepts_masked_batches():
    evaluate_mod._check_batch(_batch(0, mask=True), "evaluate")
    with pytest.raises(ValueError, match="rgb_gt"):
        evaluate_mod._check_batch(_batch(0, mask=True, gt=False), "evaluate")
    assert "mask" in evaluate_mod.evaluate.__doc__
