"""Torch-facing wrapper of the Euclidean distance field (include/lsf_hip.h: lsf_esdf_compute; INTEGRATION.md section 3,
"Euclidean distance field"; tests/esdf_restatement.py restates it): the exact squared lattice distance of every voxel to
the nearest site of the model's zero crossing, capped at max_distance_voxels, the site's flat index and the signed
metric field.  Every argument is checked on the host before a launch.  An Esdf object owns the two int32 scratch volumes
and the record, kept from call to call while the shape stays; a call enqueues one fill and three launches and reads the
record back, its one host synchronisation.  The public interface is fusion.CanonicalVolume.esdf and
fusion.SequenceFusion3d.esdf."""
import ctypes
import math
import operator

import torch

from . import _lib
from ._lib import EsdfParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_fusion import check_model

RECORD_FIELDS = _lib.ESDF_RECORD_FIELDS
FAR = _lib.ESDF_FAR
INT32_MAX = 0x7fffffff


def params(shape, voxel_size=0.004, max_distance_voxels=32, iso=0.0, min_weight=0.0, unknown="free",
           passes=_lib.ESDF_PASSES_ALL):
    """the lsf_esdf_params of a call, after the host checks"""
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("a distance field needs a 3-D (Z, Y, X) model, got shape %s" % (tuple(shape),))
    z, y, x = (int(v) for v in shape)
    if z * y * x > INT32_MAX:
        raise ValueError("a volume of shape %s has more voxels than the int32 indices of `nearest` reach"
                         % (tuple(shape),))
    try:
        r = operator.index(max_distance_voxels)
    except TypeError:
        raise ValueError("max_distance_voxels must be an integer, got %r" % (max_distance_voxels,)) from None
    if isinstance(max_distance_voxels, bool) or not 1 <= r <= _lib.ESDF_MAX_DISTANCE:
        raise ValueError("max_distance_voxels must be an integer in 1 .. %d, got %r"
                         % (_lib.ESDF_MAX_DISTANCE, max_distance_voxels))
    if unknown not in _lib.ESDF_UNKNOWN:
        raise ValueError("unknown must be 'free' or 'occupied', got %r" % (unknown,))
    size = float(voxel_size)
    if not (math.isfinite(size) and size > 0):
        raise ValueError("voxel_size must be finite and positive, got %r" % (voxel_size,))
    if math.isnan(float(iso)) or math.isnan(float(min_weight)):
        raise ValueError("iso and min_weight must not be NaN, got %r and %r" % (iso, min_weight))
    if not 1 <= int(passes) <= _lib.ESDF_PASSES_ALL:
        raise ValueError("passes must be a non-empty set of the pass bits, got %r" % (passes,))
    p = EsdfParams()
    p.voxel_size, p.iso, p.min_weight = size, float(iso), float(min_weight)
    p.depth, p.height, p.width = z, y, x
    p.max_distance_voxels, p.unknown, p.passes = r, _lib.ESDF_UNKNOWN[unknown], int(passes)
    return p


def unpack_record(record):
    """{field: int} of a host copy of the record"""
    return dict(zip(RECORD_FIELDS, (int(x) for x in record)))


class Esdf:
    """the scratch volumes and the record of lsf_esdf_compute, allocated at the first call and again when the model's
    shape or device changes; `record` is the last call's, as a dict"""

    def __init__(self):
        self._scratch = None
        self._record = None
        self.record = None

    def _workspace(self, like):
        s = self._scratch
        if s is None or s[0].shape != like.shape or s[0].device != like.device:
            self._scratch = tuple(torch.empty(like.shape, dtype=torch.int32, device=like.device) for _ in range(2))
            self._record = torch.empty(_lib.ESDF_RECORD_WORDS, dtype=torch.int64, device=like.device)
        return self._scratch

    def enqueue(self, tsdf, weight, p, outputs=None):
        """the launches of lsf_esdf_compute under params p, without a wait; outputs (distance2, nearest, esdf) are
        allocated unless given"""
        require_gpu()
        if tsdf is not None and hasattr(tsdf, "ndim") and tsdf.ndim != 3:
            raise ValueError("a distance field needs a 3-D (Z, Y, X) model, got shape %s" % (tuple(tsdf.shape),))
        check_model(tsdf, weight)
        if tuple(tsdf.shape) != (p.depth, p.height, p.width):
            raise ValueError("the params are for shape %s, the model has %s"
                             % ((p.depth, p.height, p.width), tuple(tsdf.shape)))
        a, b = self._workspace(tsdf)
        if outputs is None:
            outputs = (torch.empty_like(a), torch.empty_like(a), torch.empty_like(tsdf))
        for name, t, dtype in zip(("distance2", "nearest", "esdf"), outputs, (torch.int32, torch.int32, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.shape != tsdf.shape or t.device != tsdf.device \
                    or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor of the model's shape on its device"
                                 % (name, str(dtype).replace("torch.", "")))
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        check(lib.lsf_esdf_compute(ptr(tsdf), ptr(weight), ptr(a), ptr(b), *(ptr(t) for t in outputs),
                                   ptr(self._record), ctypes.byref(p), stream_ptr()), "lsf_esdf_compute")
        return outputs

    def compute(self, tsdf, weight, voxel_size=0.004, max_distance_voxels=32, iso=0.0, min_weight=0.0, unknown="free",
                outputs=None):
        """(esdf float32, distance2 int32, nearest int32, record) of the float32 contiguous device tensors tsdf and
        weight of one 3-D shape: device tensors of that shape and the record as a dict.  One host synchronisation, the
        read of the record.  outputs: (distance2, nearest, esdf) to write into instead of fresh tensors."""
        p = params(tuple(tsdf.shape) if hasattr(tsdf, "shape") else (), voxel_size, max_distance_voxels, iso,
                   min_weight, unknown)
        distance2, nearest, esdf = self.enqueue(tsdf, weight, p, outputs)
        self.record = unpack_record(self._record.tolist())  # the call's one host synchronisation
        return esdf, distance2, nearest, self.record
