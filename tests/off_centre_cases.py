"""Views whose rays do not start at the sensor position, shared by tests/test_cpu_off_centre_cases.py (the preconditions, on the
CPU oracle and float64 alone) and tests/test_gpu_off_centre_rays.py (the same views on the device).

Every compositing kernel and the walk are instantiated twice on the block-uniform fact "all 256 rays of this tile have the origin
(0, 0, 0) in the sensor frame" (gut_render_common.h: make_ray sets `centred`; the tile takes the un-centred form as soon as one of
its rays has another origin).  cams.pinhole_rays / fisheye_rays return an all-zero origin plane, so a view made by
common.make_view runs the centred instantiations only.  `off_centre(view, plane)` returns a copy of such a view with one of four
origin planes, float32 in the sensor frame, shape and dtype as make_view gives them:

  plane            origins                                                    tiles that take the un-centred form
  shift            the constant (0.05, -0.03, 0.02)                           all
  sweep            (0.002 (py - H/2), 0.001 (px - W/2), 0): no two rows or     all (for even W and H the ray of pixel (W/2, H/2) alone
                   columns share an origin                                    starts at the sensor: its tile is mixed)
  half             zero for px < 40, the shift elsewhere                      tile columns 0 and 1 (px 0..31): centred; column 2
                                                                              (px 32..47): mixed, un-centred; columns >= 3: un-centred
  negative_zero    -0.0f everywhere                                           none (-0.0f == 0.0f): the centred form

K1 reads no rays: the tile lists, keys and projection floats of a view do not depend on its plane."""
import numpy as np

SHIFT = (0.05, -0.03, 0.02)
HALF_CUT = 40                      # first off-centre pixel column of the `half` plane: inside the tile column 32..47
PLANES = ("shift", "sweep", "half", "negative_zero")


def origin_plane(plane, W, H):
    """The [1,H,W,3] float32 origin plane `plane` of a W x H image."""
    ro = np.zeros((1, H, W, 3), np.float32)
    if plane == "shift":
        ro[...] = np.asarray(SHIFT, np.float32)
    elif plane == "sweep":
        py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        ro[0, ..., 0] = (0.002 * (py - H / 2)).astype(np.float32)
        ro[0, ..., 1] = (0.001 * (px - W / 2)).astype(np.float32)
    elif plane == "half":
        ro[0, :, HALF_CUT:] = np.asarray(SHIFT, np.float32)
    elif plane == "negative_zero":
        ro[...] = np.float32(-0.0)
    else:
        raise KeyError(plane)
    return ro


def off_centre(view, plane):
    """A copy of the make_view result `view` with the origin plane `plane`; everything else (directions, camera, pose) is shared."""
    ro0 = view["ro"]
    ro = origin_plane(plane, view["W"], view["H"])
    assert ro.shape == ro0.shape and ro.dtype == ro0.dtype
    return dict(view, ro=np.ascontiguousarray(ro))


def uncentred_tiles(view):
    """[grid_y, grid_x] bool: the tiles the kernels run in their un-centred form — those with a ray whose origin is not == 0
    (NaN counts: NaN == 0 is false)."""
    W, H = view["W"], view["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    off = ~(view["ro"].reshape(H, W, 3) == 0).all(-1)
    out = np.zeros((gy, gx), bool)
    for ty in range(gy):
        for tx in range(gx):
            out[ty, tx] = off[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16].any()
    return out
