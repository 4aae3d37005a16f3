"""The optimiser call layer's row ranges (3dgrut_amd/optim_calls.py) on CPU tensors: a range is a slice, and the two ABI structs of
a range start at the range's first wave and always carry the overrun word.  600 rows: no multiple of 256, a partial last wave."""
import importlib
import types

import pytest
import torch

capi = importlib.import_module("3dgrut_amd._capi")
calls = importlib.import_module("3dgrut_amd.optim_calls")
native = importlib.import_module("3dgrut_amd.native")

N = 600
CHUNKS = [(0, 256), (256, 512), (512, 600)]
WAVES = (N + 63) // 64


def _trainer():
    """The tensors of a NativeTrainStep for N rows, on the CPU, with just what _lazy() / _regularisation() read."""
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    st = native.NativeTrainStep.__new__(native.NativeTrainStep)
    st.model = types.SimpleNamespace(raw=z(N, 12), features=z(N, 48), num_gaussians=N)
    st.m12, st.v12, st.m48, st.v48 = z(N, 12), z(N, 12), z(N, 48), z(N, 48)
    st.act, st.g12 = z(N, 12), z(N, 12)
    st.lazy_moments, st.LAZY_TABLE = True, 1024
    st.wave_step = z(WAVES, dtype=torch.int32)
    st._pow1, st._pow2 = z(1024), z(1024)
    st._lazy_overrun = z(1, dtype=torch.int32)
    st._reg_partials = z(WAVES, 2)
    st.lambda_opacity, st.lambda_scale = 0.01, 0.02
    return st


@pytest.mark.parametrize("r0,r1", CHUNKS)
def test_a_row_range_is_a_slice(r0, r1):
    st = _trainer()
    vis = torch.zeros(N)
    tensors = (*st._state(), st.act, st.g12, vis)
    assert [t.shape[1] if t.dim() == 2 else 1 for t in tensors] == [12, 12, 12, 48, 48, 48, 12, 12, 1]
    views = calls.rows(r0, r1, *tensors, None)
    assert views[-1] is None and len(views) == len(tensors) + 1
    for t, v in zip(tensors, views):
        assert v.shape[0] == r1 - r0 and v.is_contiguous()
        assert v.data_ptr() == t[r0:r1].data_ptr() == t.data_ptr() + r0 * t.stride(0) * t.element_size()


@pytest.mark.parametrize("r0,r1", CHUNKS)
def test_lazy_moments_of_a_row_range(r0, r1):
    st = _trainer()
    lz = st._lazy(r0)
    assert lz.d_wave_step == st.wave_step[r0 // 64:].data_ptr() == st.wave_step.data_ptr() + 4 * (r0 // 64)
    assert (lz.d_pow_beta1, lz.d_pow_beta2, lz.table_len) == (st._pow1.data_ptr(), st._pow2.data_ptr(), 1024)
    assert lz.d_overrun and lz.d_overrun == st._lazy_overrun.data_ptr()
    whole = st._lazy()
    assert whole.d_wave_step == st.wave_step.data_ptr() and whole.d_overrun == st._lazy_overrun.data_ptr()


@pytest.mark.parametrize("r0,r1", CHUNKS)
def test_regularisation_of_a_row_range(r0, r1):
    st = _trainer()
    reg = st._regularisation(r0)
    assert reg.d_partials == st._reg_partials[r0 // 64:].data_ptr() == st._reg_partials.data_ptr() + 8 * (r0 // 64)
    assert reg.density_coeff == pytest.approx(0.01 / N, rel=1e-6) and reg.scale_coeff == pytest.approx(0.02 / (3 * N), rel=1e-6)
    assert calls.regularisation(1.0, 1.0, None, r0).d_partials is None


def test_a_range_starts_on_a_wave_and_the_check_names_the_call():
    st = _trainer()
    with pytest.raises(ValueError):
        st._lazy(100)
    with pytest.raises(ValueError):
        st._regularisation(100)
    st.lazy_moments = False
    assert st._lazy(256) is None
    st.lambda_opacity = st.lambda_scale = 0.0
    assert st._regularisation(256) is None
    calls.check(0, "sh_adam_step")
    with pytest.raises(RuntimeError, match=r"\[3dgut\] sh_adam_step failed \(3\)"):
        calls.check(3, "sh_adam_step")
