"""Torch-facing wrapper of lsf_term_gradient (device.py re-exports it): one energy term of the Slavcheva-style optimizer
on its own -- data, Tikhonov, Killing or level set -- over a whole field, its narrow-band union, or a list of voxels.
The public drop-ins of nonrigid_opt/slavcheva/{data_term,smoothing_term,level_set_term}.py are built on term_field and
term_at."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import TermParams, check, lib
from .device_core import _ptr, make_grid, n_voxels, require_gpu, stream_ptr

DATA_TERMS = (_lib.TERM_DATA_BASIC, _lib.TERM_DATA_THRESHOLDED_FDM)


def term_gradient(term, grid, live=None, canonical=None, live_gradients=(), warp=None, gradient_out=None,
                  energy_out=None, energy_total=None, selection=_lib.SELECT_ALL, indices=None, interleaved=True,
                  copy_if_zero=False, ignore_if_zero=False, isomorphic_enforcement_factor=0.1, epsilon=1e-5,
                  scaling_factor=10.0, energy_form=_lib.TERM_ENERGY_LOCAL):
    """one launch of lsf_term_gradient on device tensors.  live_gradients: the caller's gradient planes (x, y[, z]),
    read by the data terms when gradient_out is given.  Outputs (each optional): gradient_out float32 (planar
    [D, count] or interleaved [count, D]), energy_out float64 [count], energy_total float64 [1] (added to).  count = the
    number of voxels, or of `indices` (int32 flat voxel indices) with SELECT_LIST."""
    n = n_voxels(grid)
    d = grid.dims
    count = int(indices.numel()) if selection == _lib.SELECT_LIST else n
    gradients = list(live_gradients) + [None] * (3 - len(live_gradients))
    flags = ((_lib.TERM_COPY_IF_ZERO if copy_if_zero else 0) | (_lib.TERM_IGNORE_IF_ZERO if ignore_if_zero else 0)
             | (_lib.TERM_INTERLEAVED if interleaved else 0))
    lam = float(isomorphic_enforcement_factor)
    params = TermParams(lam, lam, float(epsilon), float(scaling_factor), int(term), flags, 0)
    check(lib.lsf_term_gradient(_ptr(live, n, "live", allow_none=True), _ptr(canonical, n, "canonical", allow_none=True),
                                *[_ptr(g, n, "live_gradient_" + "xyz"[c], allow_none=True) for c, g in enumerate(gradients)],
                                _ptr(warp, n * d, "warp", allow_none=True),
                                _ptr(gradient_out, count * d, "gradient_out", allow_none=True),
                                _ptr(energy_out, count, "energy_out", torch.float64, allow_none=True),
                                _ptr(energy_total, 1, "energy_total", torch.float64, allow_none=True),
                                ctypes.byref(grid), ctypes.byref(params), int(selection), int(energy_form),
                                _ptr(indices, count, "indices", torch.int32, allow_none=True), count, stream_ptr()),
          "lsf_term_gradient")


# ------------------------------------------------------------------------------- numpy / tensor plumbing of the drop-ins
def _device(x, shape=None, name="field"):
    """numpy array or tensor -> contiguous float32 tensor on the current ROCm device; shape checked when given"""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t = (x if x.is_cuda else x.to("cuda")).to(torch.float32).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to("cuda")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _spatial(live, warp):
    """spatial shape of the call, from the live field or the warp (..., D)"""
    if live is not None:
        shape = tuple(live.shape)
    else:
        shape = tuple(warp.shape[:-1])
        if warp.shape[-1] != len(shape):
            raise ValueError("warp field: expected shape (..., %d), got %s" % (len(shape), tuple(warp.shape)))
    if len(shape) not in (2, 3):
        raise ValueError("fields must be 2-D or 3-D, got shape %s" % (shape,))
    return shape


def term_field(term, live=None, canonical=None, live_gradients=(), warp=None, band=False, want_gradient=True,
               want_energy=False, **options):
    """the term over a whole field (band: its narrow-band union, zeros elsewhere), ONE launch.  Inputs numpy or tensors;
    returns (gradient (..., D) float32 or None, energy total float or None) -- the gradient a tensor on the device when
    a field is given as a tensor, a numpy array otherwise; only the energy total waits for the device."""
    require_gpu()
    as_tensor = any(isinstance(f, torch.Tensor) for f in (live, canonical, warp))
    shape = _spatial(live, warp)
    d = len(shape)
    if d == 3 and (options.get("copy_if_zero") or options.get("ignore_if_zero")):
        raise ValueError("copy_if_zero / ignore_if_zero have 2-D semantics only (smoothing_term.py:50-139)")
    live_t = _device(live, shape, "warped_live_field")
    canonical_t = _device(canonical, shape, "canonical_field")
    warp_t = _device(warp, shape + (d,), "warp_field")
    gradients = []
    if want_gradient and term in DATA_TERMS:
        if len(live_gradients) < d or any(g is None for g in live_gradients[:d]):
            raise ValueError("the data term needs the live field's gradient along each of the %d axes" % d)
        gradients = [_device(g, shape, "live_gradient_" + "xyz"[c]) for c, g in enumerate(live_gradients[:d])]
    device = (live_t if live_t is not None else warp_t).device
    out = torch.empty(shape + (d,), dtype=torch.float32, device=device) if want_gradient else None
    total = torch.zeros(1, dtype=torch.float64, device=device) if want_energy else None
    term_gradient(term, make_grid(shape), live_t, canonical_t, gradients, warp_t, gradient_out=out, energy_total=total,
                  selection=_lib.SELECT_BAND if band else _lib.SELECT_ALL, interleaved=True, **options)
    if out is not None and not as_tensor:
        out = out.cpu().numpy()
    return out, (float(total.item()) if total is not None else None)


def term_at(term, x, y, live=None, canonical=None, live_gradients=(), warp=None, **options):
    """the term at one location (x, y) of a 2-D field: ONE launch and ONE wait for the device.  Returns (gradient (2,)
    float32 -- numpy, or a device tensor when a field is given as a tensor --, local energy float)."""
    require_gpu()
    as_tensor = any(isinstance(f, torch.Tensor) for f in (live, canonical, warp))
    shape = _spatial(live, warp)
    if len(shape) != 2:
        raise ValueError("the per-location term functions are 2-D (as in the reference), got shape %s" % (shape,))
    h, w = shape
    x, y = int(x), int(y)
    if not (0 <= x < w and 0 <= y < h):
        raise IndexError("location (x=%d, y=%d) is outside a field of shape %s" % (x, y, shape))
    live_t = _device(live, shape, "warped_live_field")
    canonical_t = _device(canonical, shape, "canonical_field")
    warp_t = _device(warp, shape + (2,), "warp_field")
    gradients = [_device(g, shape, "live_gradient_" + "xy"[c]) for c, g in enumerate(live_gradients[:2])] \
        if term in DATA_TERMS else []
    device = (live_t if live_t is not None else warp_t).device
    index = torch.tensor([y * w + x], dtype=torch.int32, device=device)
    result = torch.empty(16, dtype=torch.uint8, device=device)  # gradient (2 x float32), then the energy (float64)
    gradient, energy = result[:8].view(torch.float32), result[8:].view(torch.float64)
    term_gradient(term, make_grid(shape), live_t, canonical_t, gradients, warp_t, gradient_out=gradient,
                  energy_out=energy, selection=_lib.SELECT_LIST, indices=index, interleaved=True, **options)
    host = result.cpu()
    value = float(host[8:].view(torch.float64)[0])
    if as_tensor:
        return gradient, value
    return host[:8].view(torch.float32).numpy().copy(), value
