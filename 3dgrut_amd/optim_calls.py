"""The one place that calls each handle-less optimiser entry point of libgut_hip.so (include/gut_hip.h).

Every function takes the loaded library, the stream (its integer handle) and TENSORS; the pointer handed to the library is the
tensor's data_ptr().  A row range is a slice: `rows(r0, r1, ...)` returns the `t[r0:r1]` views, `lazy_moments(..., r0)` and
`regularisation(..., r0)` build the two ABI structs for a range that starts at row r0 (a multiple of 64: whole waves).  Nothing
outside this module does pointer arithmetic on optimiser state.

  state : (raw12, raw_m, raw_v, sh48, sh_m, sh_v) — the [N,12] and [N,48] parameters with their two moments each
  adam  : (lr12, lr48, betas, eps, step) — float32 numpy learning rates per column, (beta1, beta2), eps, the 1-based step being
          applied (0 = no bias correction)

These entry points do not set gut_last_error(): their return code goes through check() below, which never prints a stale message
(_capi.check stays the check of the calls on a handle).
"""
import ctypes as C

from . import _capi

_F32P = C.POINTER(C.c_float)
WAVE = 64   # rows per wave: the granularity of wave_step and of the regularisers' loss partials


def check(rc, what):
    if rc:
        raise RuntimeError(f"[3dgut] {what} failed ({rc})")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ref(struct):
    return None if struct is None else C.byref(struct)


def rows(r0, r1, *tensors):
    """The rows [r0, r1) of every tensor, as views (None stays None)."""
    return tuple(None if t is None else t[r0:r1] for t in tensors)


def lazy_moments(wave_step, pow1, pow2, table_len, overrun, r0=0):
    """GutLazyMoments for the rows from r0 on (a multiple of 64): wave_step advanced by r0 / 64 words, the tables and the overrun
    word as they are.  The overrun word always travels: without it a wave beyond the tables is clamped silently."""
    if r0 % WAVE:
        raise ValueError("a row range of the lazy moment decay starts at a multiple of 64")
    first = wave_step if r0 == 0 else wave_step[r0 // WAVE:]
    return _capi.GutLazyMoments(first.data_ptr(), pow1.data_ptr(), pow2.data_ptr(), int(table_len), overrun.data_ptr())


def regularisation(density_coeff, scale_coeff, partials, r0=0):
    """GutRegularisation for the rows from r0 on (a multiple of 64): partials [waves, 2] advanced by r0 / 64 pairs (or None)."""
    if r0 % WAVE:
        raise ValueError("a row range of the regularisers starts at a multiple of 64")
    first = partials if (r0 == 0 or partials is None) else partials[r0 // WAVE:]
    return _capi.GutRegularisation(density_coeff, scale_coeff, _ptr(first))


def sh_adam_step(lib, stream, state, adam, sh_degree, cams, mrgb, g12, grad_scale, act, visibility=None, flags=0, wave_flags=None,
                 lazy=None, reg=None):
    """gut_sh_adam_step_regularised over the rows of `state` (all of them, or a rows() range with mrgb [views, rows, 3], g12,
    visibility and act sliced alike): SH-gradient rebuild from the views' compact radiance gradients + Adam."""
    raw12, raw_m, raw_v, sh48, sh_m, sh_v = state
    lr12, lr48, betas, eps, step = adam
    n = raw12.shape[0]
    check(lib.gut_sh_adam_step_regularised(
        C.c_void_p(stream), n, sh_degree, cams.shape[0], cams.data_ptr(), mrgb.data_ptr(), g12.data_ptr(), grad_scale,
        raw12.data_ptr(), raw_m.data_ptr(), raw_v.data_ptr(), sh48.data_ptr(), sh_m.data_ptr(), sh_v.data_ptr(),
        lr12.ctypes.data_as(_F32P), lr48.ctypes.data_as(_F32P), betas[0], betas[1], eps, step, _ptr(visibility), act.data_ptr(), n,
        flags, _ptr(wave_flags), _ref(lazy), _ref(reg)), "sh_adam_step")


def adam_unwalked_waves(lib, stream, wave_flags, state, adam, act, lazy=None, reg=None):
    """gut_adam_unwalked_waves_regularised: the zero-gradient Adam step of the waves whose flag is 0."""
    raw12, raw_m, raw_v, sh48, sh_m, sh_v = state
    lr12, lr48, betas, eps, step = adam
    check(lib.gut_adam_unwalked_waves_regularised(
        C.c_void_p(stream), raw12.shape[0], wave_flags.data_ptr(), raw12.data_ptr(), raw_m.data_ptr(), raw_v.data_ptr(),
        sh48.data_ptr(), sh_m.data_ptr(), sh_v.data_ptr(), lr12.ctypes.data_as(_F32P), lr48.ctypes.data_as(_F32P), betas[0], betas[1],
        eps, step, act.data_ptr(), _ref(lazy), _ref(reg)), "adam_unwalked_waves")


def sync_moments(lib, stream, raw_m, raw_v, sh_m, sh_v, lazy, step, reg=None):
    """gut_sync_moments_ex: every stored moment brought up to `step` (reg on: only the [N,48] block, the [N,12] one is current)."""
    check(lib.gut_sync_moments_ex(C.c_void_p(stream), raw_m.shape[0], raw_m.data_ptr(), raw_v.data_ptr(), sh_m.data_ptr(),
                                  sh_v.data_ptr(), C.byref(lazy), step, _ref(reg)), "sync_moments")


def regularisation_gradient(lib, stream, raw12, g12, reg):
    """gut_regularisation_gradient: the regularisers' gradient of the rows of raw12 added to g12."""
    check(lib.gut_regularisation_gradient(C.c_void_p(stream), raw12.shape[0], raw12.data_ptr(), g12.data_ptr(), C.byref(reg)),
          "regularisation_gradient")


def regularisation_loss(lib, stream, n, partials, lambda_opacity, lambda_scale, opacity_loss, scale_loss, loss_buffer=None):
    """gut_regularisation_loss: the two loss values (device scalars) from the per-wave partials; also added to loss_buffer[0]."""
    check(lib.gut_regularisation_loss(C.c_void_p(stream), n, partials.data_ptr(), lambda_opacity, lambda_scale,
                                      opacity_loss.data_ptr(), scale_loss.data_ptr(), _ptr(loss_buffer)), "regularisation_loss")


def scatter_gradient_records(lib, stream, records, count, g12, mrgb_view):
    """gut_scatter_gradient_records: the first `count` (host integer) records added into g12 [N,12] and mrgb_view [N,3]."""
    check(lib.gut_scatter_gradient_records(C.c_void_p(stream), records.data_ptr(), count, g12.shape[0], g12.data_ptr(),
                                           mrgb_view.data_ptr()), "scatter_gradient_records")


def scatter_gradient_records_dev(lib, stream, records, counts, view, capacity, g12, mrgb_view):
    """gut_scatter_gradient_records_dev: as above with the count read on the device, from counts[view], at most `capacity`."""
    check(lib.gut_scatter_gradient_records_dev(C.c_void_p(stream), records.data_ptr(), counts.data_ptr() + view * counts.element_size(),
                                               capacity, g12.shape[0], g12.data_ptr(), mrgb_view.data_ptr()),
          "scatter_gradient_records")


def activate_pack(lib, stream, raw12, act):
    """gut_activate_pack: act := the activated rows of raw12."""
    check(lib.gut_activate_pack(C.c_void_p(stream), raw12.shape[0], raw12.data_ptr(), act.data_ptr()), "activate_pack")


def adam_step(lib, stream, p, g, m, v, lr, betas, eps, step, visibility=None):
    """gut_adam_step on one [N,C] tensor with per-column learning rates `lr` (C floats)."""
    lr_arr = (C.c_float * len(lr))(*[float(x) for x in lr])
    check(lib.gut_adam_step(C.c_void_p(stream), p.shape[0], p.shape[1], p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), lr_arr,
                            betas[0], betas[1], eps, step, _ptr(visibility)), "adam_step")
