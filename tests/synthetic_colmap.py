"""A synthetic COLMAP scene for the trainer tests: a teacher (scenes.scene_lego_like) rendered with the HIP forward from orbit views,
saved as PNG under images/, and sparse/0 written with io_colmap.write_model_binary (PINHOLE camera, jittered teacher points and
their colours as points3D)."""
import importlib
import os

import numpy as np
import torch

cams = importlib.import_module("3dgrut_amd.cameras")
io_colmap = importlib.import_module("3dgrut_amd.io_colmap")
native = importlib.import_module("3dgrut_amd.native")
scenes = importlib.import_module("3dgrut_amd.scenes")
Batch = importlib.import_module("3dgrut_amd.protocols").Batch
SH_C0 = 0.28209479177387814


def write_synthetic_colmap(root, n_views=32, size=400, n_teacher=200_000, n_points=20_000, radius=4.0, seed=0):
    from PIL import Image
    gut = importlib.import_module("3dgrut_amd")
    teacher = scenes.scene_lego_like(n_teacher, seed=seed + 1)
    model = native.NativeGaussianModel(teacher, device="cuda")
    tracer = gut.Tracer({"render": {}})
    f = 0.9 * size
    ro, rd = cams.pinhole_rays(size, size, f, f)
    K = cams.pinhole_intrinsics_dict(size, size, f, f)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    images = []
    with torch.no_grad():
        for i in range(n_views):
            c2w = cams.orbit_c2w(radius, 360.0 * i / n_views, 10.0 + 25.0 * (i % 4) / 3.0)
            batch = Batch(rays_ori=torch.as_tensor(ro, device="cuda"), rays_dir=torch.as_tensor(rd, device="cuda"),
                          T_to_world=torch.as_tensor(c2w, device="cuda")[None], intrinsics_OpenCVPinholeCameraModelParameters=K)
            rgb = tracer.render(model, batch, train=False)["pred_rgb"][0]
            img = rgb.mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy()
            name = f"{i:03d}.png"
            Image.fromarray(img).save(os.path.join(root, "images", name))
            w2c = np.linalg.inv(c2w.astype(np.float64))
            images.append(io_colmap.ColmapImage(i + 1, io_colmap.rotation_to_qvec(w2c[:3, :3]), w2c[:3, 3], 1, name))
    rng = np.random.default_rng(seed)
    pick = rng.choice(n_teacher, size=n_points, replace=False)
    xyz = teacher["positions"][pick] + rng.normal(0.0, 0.01, size=(n_points, 3))
    rgb = np.clip(0.5 + SH_C0 * teacher["features"][pick, 0:3], 0.0, 1.0)
    camera = io_colmap.ColmapCamera(1, "PINHOLE", size, size, np.array([f, f, size / 2, size / 2], np.float64))
    io_colmap.write_model_binary(os.path.join(root, "sparse", "0"), {1: camera}, images, xyz, (rgb * 255 + 0.5).astype(np.uint8))
    del model, tracer
    torch.cuda.empty_cache()
    return root


def load_scene(root, test_split_interval=8):
    """(initial Gaussians, train batches, test batches, scene extent) as the trainer's CLI builds them."""
    train = io_colmap.ColmapScene(root, "train", 1, test_split_interval)
    test = io_colmap.ColmapScene(root, "test", 1, test_split_interval)
    init = train.initial_gaussians(use_observation_points=True)
    return init, [train.batch(i) for i in range(len(train))], [test.batch(i) for i in range(len(test))], train.cameras_extent
