"""GutPhotometricLoss / gut_photometric_loss_run without a GPU: the descriptor's layout as include/gut_hip.h declares it, and the
refusals, which return 1 on the host before anything is queued (as tests/test_cpu_exposure.py relies on for the positional forms)."""
import ctypes as C
import importlib

import pytest

capi = importlib.import_module("3dgrut_amd._capi")

POINTERS = ["d_rgba", "d_gt_rgb", "d_mask", "d_background", "d_exposure12", "d_workspace", "d_loss3", "d_rgba_grad", "d_exposure_grad12"]
FLOATS = ["background", "lambda_l1", "lambda_ssim"]
REQUIRED = ["d_rgba", "d_gt_rgb", "d_workspace", "d_loss3", "d_rgba_grad"]


def _descriptor(buf, **over):
    """Every pointer set (to host memory: nothing is dereferenced on the host), then the overrides."""
    p = C.addressof(buf)
    fields = dict({name: p for name in POINTERS}, background=0.0, lambda_l1=0.8, lambda_ssim=0.2)
    fields.update(over)
    return capi.GutPhotometricLoss(**fields)


def test_descriptor_layout_is_the_headers():
    D = capi.GutPhotometricLoss
    assert C.sizeof(D) == 88
    assert [name for name, _ in D._fields_] == POINTERS + FLOATS
    assert all(ctype is C.c_void_p for _, ctype in D._fields_[:9]) and all(ctype is C.c_float for _, ctype in D._fields_[9:])
    assert [getattr(D, name).offset for name in POINTERS] == [8 * i for i in range(9)]
    assert [getattr(D, name).offset for name in FLOATS] == [72, 76, 80]


def test_entry_point_is_exported_and_declared():
    lib = capi.load()
    assert "gut_photometric_loss_run" in capi.EXPORTS and hasattr(lib, "gut_photometric_loss_run")
    assert len(lib.gut_photometric_loss_run.argtypes) == 4
    assert lib.gut_abi_version() == 6 == capi.GUT_ABI_VERSION


def test_null_descriptor_is_refused():
    assert capi.load().gut_photometric_loss_run(None, 37, 53, None) == 1


@pytest.mark.parametrize("name", REQUIRED)
def test_each_null_required_pointer_is_refused(name):
    buf = (C.c_float * 16)()
    assert capi.load().gut_photometric_loss_run(None, 37, 53, C.byref(_descriptor(buf, **{name: None}))) == 1


def test_images_of_ten_pixels_either_way_are_refused():
    lib = capi.load()
    buf = (C.c_float * 16)()
    d = _descriptor(buf)
    assert lib.gut_photometric_loss_run(None, 10, 53, C.byref(d)) == 1
    assert lib.gut_photometric_loss_run(None, 37, 10, C.byref(d)) == 1


def test_gradient_output_without_an_exposure_is_refused():
    buf = (C.c_float * 16)()
    d = _descriptor(buf, d_exposure12=None)
    assert d.d_exposure_grad12 is not None
    assert capi.load().gut_photometric_loss_run(None, 37, 53, C.byref(d)) == 1
