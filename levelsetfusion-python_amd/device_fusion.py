"""Torch-facing wrapper of the fusion entry points (include/lsf_hip.h: lsf_fusion_integrate_volume,
lsf_fusion_integrate_depth, lsf_fusion_integrate_depth_weighted, lsf_fusion_integrate_depth_colour,
lsf_fusion_integrate_depth_warped).  Every argument is checked on the host before a launch; a call enqueues two launches
and returns the record as a device tensor without waiting for it -- the caller decides when to copy it back.  The public
interface is fusion.CanonicalVolume / fusion.SequenceFusion3d."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import FusionColourParams, FusionParams, FusionWarpedParams, FusionWeightedParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_rigid import _tsdf3d, twist6
from .tsdf.generation import offsets_of

RECORD = _lib.FUSION_RECORD_DOUBLES
RECORD_FIELDS = ("fused", "first_seen", "sum_abs_change", "max_abs_change")
WEIGHTED_RECORD_FIELDS = RECORD_FIELDS + ("carved", "weight_rejected")
COLOUR_RECORD_FIELDS = WEIGHTED_RECORD_FIELDS + ("coloured", "first_coloured")
WARPED_RECORD = _lib.FUSION_WARPED_RECORD_DOUBLES
WARPED_RECORD_FIELDS = COLOUR_RECORD_FIELDS + ("warp_rejected",)


def fusion_weights(weight, max_weight):
    """(w, max_weight) as float32 values after the rule's checks: w finite and > 0, max_weight > 0 (inf allowed)"""
    with np.errstate(over="ignore"):
        w, cap = np.float32(weight), np.float32(max_weight)
    if not (np.isfinite(w) and w > 0):
        raise ValueError("weight must be finite and > 0 as a float32, got %r" % (weight,))
    if not cap > 0:
        raise ValueError("max_weight must be > 0 (inf allowed), got %r" % (max_weight,))
    return float(w), float(cap)


def _overlap(a, b):
    sa = a.untyped_storage().data_ptr(), a.untyped_storage().nbytes()
    sb = b.untyped_storage().data_ptr(), b.untyped_storage().nbytes()
    if sa[0] == sb[0]:
        lo_a, lo_b = a.data_ptr(), b.data_ptr()
        return lo_a < lo_b + b.numel() * b.element_size() and lo_b < lo_a + a.numel() * a.element_size()
    return False


def check_model(tsdf, weight, live=None):
    """the model buffers (and a live field): float32, contiguous, on the GPU, one device, one shape, no aliasing"""
    named = [("tsdf", tsdf), ("weight", weight)] + ([("live", live)] if live is not None else [])
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, t.dtype))
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    for name, t in named[1:]:
        if t.device != tsdf.device:
            raise ValueError("%s is on %s, tsdf on %s: all buffers must be on one device" % (name, t.device,
                                                                                             tsdf.device))
        if tuple(t.shape) != tuple(tsdf.shape):
            raise ValueError("%s has shape %s, tsdf %s: they must have one shape" % (name, tuple(t.shape),
                                                                                    tuple(tsdf.shape)))
    if tsdf.numel() == 0:
        raise ValueError("the volume is empty")
    if _overlap(tsdf, weight):
        raise ValueError("tsdf and weight must be distinct buffers")
    if live is not None and (_overlap(live, tsdf) or _overlap(live, weight)):
        raise ValueError("live must not alias tsdf or weight")


def _params(shape, weight, max_weight):
    p = FusionParams()
    w, cap = fusion_weights(weight, max_weight)
    p.weight, p.max_weight = w, cap
    n = int(np.prod(shape))
    if len(shape) == 3:
        p.depth, p.height, p.width = (int(s) for s in shape)
    else:  # the volume mode's index is flat: any shape is one run of voxels
        p.depth, p.height, p.width = 1, 1, n
    return p


def _record_and_scratch(tsdf, record, scratch_bytes):
    record = torch.empty(RECORD, dtype=torch.float64, device=tsdf.device) if record is None else record
    return record, torch.empty(scratch_bytes // 8, dtype=torch.float64, device=tsdf.device)


def _launch(fn, name, tsdf, weight, source, p, record):
    record, scratch = _record_and_scratch(tsdf, record, _lib.FUSION_SCRATCH_BYTES)
    check(fn(ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr()), ctypes.c_void_p(source.data_ptr()),
             ctypes.c_void_p(record.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), ctypes.byref(p), stream_ptr()),
          name)
    return record


def integrate_volume(tsdf, weight, live, w=1.0, max_weight=math.inf, record=None):
    """fuse the live field into (tsdf, weight) in place, one launch and a finishing one; returns the record, a float64
    device tensor of RECORD doubles (unpack_record once it is on the host)"""
    require_gpu()
    check_model(tsdf, weight, live)
    p = _params(tuple(tsdf.shape), w, max_weight)
    return _launch(lib.lsf_fusion_integrate_volume, "lsf_fusion_integrate_volume", tsdf, weight, live, p, record)


def _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                  narrow_band_width_voxels, w, max_weight, default_value):
    """the checks of a depth-mode call and its lsf_fusion_params"""
    check_model(tsdf, weight)
    if tsdf.dim() != 3:
        raise ValueError("depth mode fuses a 3-D (Z, Y, X) volume, got shape %s" % (tuple(tsdf.shape),))
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dim() != 2 or not depth.is_contiguous():
        raise ValueError("depth must be a contiguous 2-D device tensor (tsdf.generation.device_depth)")
    if depth.device != tsdf.device:
        raise ValueError("depth is on %s, tsdf on %s: all buffers must be on one device" % (depth.device, tsdf.device))
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    p = _params(tuple(tsdf.shape), w, max_weight)
    P = np.asarray(camera.intrinsics.intrinsic_matrix)
    p.tsdf = _tsdf3d(P, camera, depth, voxel_size, narrow_band_width_voxels, default_value)
    p.twist[:] = list(twist6(twist))
    p.array_offset[:] = list(offsets_of(array_offset))
    p.depth_dtype = int(depth_code)
    return p


def integrate_depth(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                    narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, default_value=1, record=None):
    """generate the live volume of the device depth image (uint16 / float32 / float64, depth_code LSF_DEPTH_*) under
    twist exactly as device_rigid.live_and_gradient_3d does, and fuse it into the (Z, Y, X) model in the same pass;
    returns the record as integrate_volume does"""
    require_gpu()
    p = _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                      narrow_band_width_voxels, w, max_weight, default_value)
    return _launch(lib.lsf_fusion_integrate_depth, "lsf_fusion_integrate_depth", tsdf, weight, depth, p, record)


def check_pixel_weight(pixel_weight, depth, tsdf, weight):
    """a weight image: a float32 contiguous tensor on the model's device, of the depth image's shape, aliasing neither
    the model nor the depth image"""
    if not isinstance(pixel_weight, torch.Tensor):
        raise TypeError("pixel_weight must be a torch tensor, got %s" % type(pixel_weight).__name__)
    if pixel_weight.dtype != torch.float32:
        raise ValueError("pixel_weight must be float32, got %s" % pixel_weight.dtype)
    if pixel_weight.device != tsdf.device:
        raise ValueError("pixel_weight is on %s, tsdf on %s: all buffers must be on one device"
                         % (pixel_weight.device, tsdf.device))
    if not pixel_weight.is_contiguous():
        raise ValueError("pixel_weight must be contiguous")
    if tuple(pixel_weight.shape) != tuple(depth.shape):
        raise ValueError("pixel_weight has shape %s, the depth image %s: they must have one shape"
                         % (tuple(pixel_weight.shape), tuple(depth.shape)))
    if _overlap(pixel_weight, tsdf) or _overlap(pixel_weight, weight) or _overlap(pixel_weight, depth):
        raise ValueError("pixel_weight must not alias tsdf, weight or the depth image")


def integrate_depth_weighted(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                             narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None, carve=False,
                             record=None):
    """integrate_depth with the weighted rule ("Weighted fusion and carving"): a voxel's
    weight is w times pixel_weight at the pixel it projects to (a float32 device image of depth's shape; None: w
    itself), and with carve the seen free space in front of the band (live value exactly 1 at a valid pixel) is fused
    with +1.  Two launches, no host wait; returns the record (unpack_weighted_record once it is on the host)"""
    require_gpu()
    p = FusionWeightedParams()
    p.fusion = _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                             narrow_band_width_voxels, w, max_weight, 1)
    if pixel_weight is not None:
        check_pixel_weight(pixel_weight, depth, tsdf, weight)
    p.carve, p.has_pixel_weight = int(bool(carve)), int(pixel_weight is not None)
    record, scratch = _record_and_scratch(tsdf, record, _lib.FUSION_WEIGHTED_SCRATCH_BYTES)
    check(lib.lsf_fusion_integrate_depth_weighted(
        ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr()), ctypes.c_void_p(depth.data_ptr()),
        ctypes.c_void_p(None if pixel_weight is None else pixel_weight.data_ptr()), ctypes.c_void_p(record.data_ptr()),
        ctypes.c_void_p(scratch.data_ptr()), ctypes.byref(p), stream_ptr()), "lsf_fusion_integrate_depth_weighted")
    return record


def colour_band_of(colour_band):
    """colour_band as a float32 value after the rule's check: finite and in (0, 1]"""
    band = np.float32(colour_band)
    if not (band > 0 and band <= 1):  # NaN fails
        raise ValueError("colour_band must be finite and in (0, 1], got %r" % (colour_band,))
    return float(band)


def check_colour_volume(colour, tsdf, weight):
    """a colour volume: a float32 contiguous tensor of shape tsdf.shape + (4,) on the model's device, 16-byte aligned,
    aliasing neither tsdf nor weight"""
    if not isinstance(colour, torch.Tensor):
        raise TypeError("colour must be a torch tensor, got %s" % type(colour).__name__)
    if colour.dtype != torch.float32:
        raise ValueError("colour must be float32, got %s" % colour.dtype)
    if colour.device != tsdf.device:
        raise ValueError("colour is on %s, tsdf on %s: all buffers must be on one device" % (colour.device, tsdf.device))
    if not colour.is_contiguous():
        raise ValueError("colour must be contiguous")
    if tuple(colour.shape) != tuple(tsdf.shape) + (4,):
        raise ValueError("colour has shape %s, the model %s: it must be the model's shape + (4,)"
                         % (tuple(colour.shape), tuple(tsdf.shape)))
    if colour.data_ptr() % 16:
        raise ValueError("colour must be 16-byte aligned: a voxel's record is one 16-byte access")
    if _overlap(colour, tsdf) or _overlap(colour, weight):
        raise ValueError("colour must not alias tsdf or weight")


def check_colour_image(colour_image, depth, others):
    """a colour image: a uint8 contiguous (H, W, 3) tensor on the depth image's device, H and W the depth image's,
    aliasing none of `others` ((name, tensor) pairs; None tensors are skipped)"""
    if not isinstance(colour_image, torch.Tensor):
        raise TypeError("colour_image must be a torch tensor, got %s" % type(colour_image).__name__)
    if colour_image.dtype != torch.uint8:
        raise ValueError("colour_image must be uint8, got %s" % colour_image.dtype)
    if colour_image.device != depth.device:
        raise ValueError("colour_image is on %s, the depth image on %s: all buffers must be on one device"
                         % (colour_image.device, depth.device))
    if not colour_image.is_contiguous():
        raise ValueError("colour_image must be contiguous")
    if tuple(colour_image.shape) != tuple(depth.shape) + (3,):
        raise ValueError("colour_image has shape %s, the depth image %s: it must be (H, W, 3) with the depth image's H, W"
                         % (tuple(colour_image.shape), tuple(depth.shape)))
    for name, t in others:
        if t is not None and _overlap(colour_image, t):
            raise ValueError("colour_image must not alias %s" % name)


def integrate_depth_colour(tsdf, weight, colour, depth, depth_code, camera, array_offset, twist, colour_image,
                           voxel_size=0.004, narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None,
                           carve=False, colour_band=1.0, record=None):
    """integrate_depth_weighted that also fuses colour_image (uint8 (H, W, 3) device tensor registered to the depth
    image) into the colour volume (float32, tsdf.shape + (4,): R, G, B in 0..255 and the colour weight) of the voxels
    whose live value lies strictly inside (-colour_band, colour_band) ("Colour fusion").
    tsdf, weight and record slots 0..5 are integrate_depth_weighted's bit for bit.  Two launches, no host wait; returns
    the record (unpack_colour_record once it is on the host)"""
    require_gpu()
    p = FusionColourParams()
    p.weighted.fusion = _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                                      narrow_band_width_voxels, w, max_weight, 1)
    if pixel_weight is not None:
        check_pixel_weight(pixel_weight, depth, tsdf, weight)
    check_colour_volume(colour, tsdf, weight)
    check_colour_image(colour_image, depth, [("tsdf", tsdf), ("weight", weight), ("colour", colour), ("depth", depth),
                                             ("pixel_weight", pixel_weight)])
    if _overlap(colour, depth) or (pixel_weight is not None and _overlap(colour, pixel_weight)):
        raise ValueError("colour must not alias the depth image or pixel_weight")
    p.weighted.carve, p.weighted.has_pixel_weight = int(bool(carve)), int(pixel_weight is not None)
    p.colour_band = colour_band_of(colour_band)
    record, scratch = _record_and_scratch(tsdf, record, _lib.FUSION_COLOUR_SCRATCH_BYTES)
    check(lib.lsf_fusion_integrate_depth_colour(
        ctypes.c_void_p(tsdf.data_ptr()), ctypes.c_void_p(weight.data_ptr()), ctypes.c_void_p(colour.data_ptr()),
        ctypes.c_void_p(depth.data_ptr()), ctypes.c_void_p(None if pixel_weight is None else pixel_weight.data_ptr()),
        ctypes.c_void_p(colour_image.data_ptr()), ctypes.c_void_p(record.data_ptr()),
        ctypes.c_void_p(scratch.data_ptr()), ctypes.byref(p), stream_ptr()), "lsf_fusion_integrate_depth_colour")
    return record


def check_warp(warp, tsdf, others):
    """a warp field: a float32 contiguous tensor of shape tsdf.shape + (3,) on the model's device (what
    HierarchicalOptimizer3d.optimize returns for device inputs), aliasing none of `others` ((name, tensor) pairs; None
    tensors are skipped)"""
    if not isinstance(warp, torch.Tensor):
        raise TypeError("warp must be a torch tensor, got %s" % type(warp).__name__)
    if warp.dtype != torch.float32:
        raise ValueError("warp must be float32, got %s" % warp.dtype)
    if warp.device != tsdf.device:
        raise ValueError("warp is on %s, tsdf on %s: all buffers must be on one device" % (warp.device, tsdf.device))
    if not warp.is_contiguous():
        raise ValueError("warp must be contiguous")
    if tuple(warp.shape) != tuple(tsdf.shape) + (3,):
        raise ValueError("warp has shape %s, the model %s: it must be the model's shape + (3,)"
                         % (tuple(warp.shape), tuple(tsdf.shape)))
    for name, t in others:
        if t is not None and _overlap(warp, t):
            raise ValueError("warp must not alias %s" % name)


def integrate_depth_warped(tsdf, weight, depth, depth_code, camera, array_offset, twist, warp, voxel_size=0.004,
                           narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None, carve=False,
                           colour=None, colour_image=None, colour_band=1.0, record=None):
    """integrate_depth_weighted -- and integrate_depth_colour, when colour and colour_image are given (both or neither)
    -- through a non-rigid warp field ("Warped depth fusion"): warp is a float32 device tensor
    of shape tsdf.shape + (3,), channel 0 the x displacement, 1 y, 2 z, in voxels; voxel v observes the frame at
    v + warp[v] in place of its centre, and a voxel whose displacement is not finite is left alone and counted.  With a
    zero warp the result equals those calls bit for bit.  Two launches, no host wait; returns the record, WARPED_RECORD
    doubles (unpack_warped_record once it is on the host)"""
    require_gpu()
    if (colour is None) != (colour_image is None):
        raise ValueError("colour and colour_image are given together or not at all")
    p = FusionWarpedParams()
    p.colour.weighted.fusion = _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                                             narrow_band_width_voxels, w, max_weight, 1)
    if pixel_weight is not None:
        check_pixel_weight(pixel_weight, depth, tsdf, weight)
    if colour is not None:
        check_colour_volume(colour, tsdf, weight)
        check_colour_image(colour_image, depth, [("tsdf", tsdf), ("weight", weight), ("colour", colour),
                                                 ("depth", depth), ("pixel_weight", pixel_weight)])
        if _overlap(colour, depth) or (pixel_weight is not None and _overlap(colour, pixel_weight)):
            raise ValueError("colour must not alias the depth image or pixel_weight")
    check_warp(warp, tsdf, [("tsdf", tsdf), ("weight", weight), ("colour", colour), ("depth", depth),
                            ("pixel_weight", pixel_weight), ("colour_image", colour_image)])
    p.colour.weighted.carve, p.colour.weighted.has_pixel_weight = int(bool(carve)), int(pixel_weight is not None)
    p.colour.colour_band = colour_band_of(colour_band)
    p.has_colour = int(colour is not None)
    if record is None:
        record = torch.empty(WARPED_RECORD, dtype=torch.float64, device=tsdf.device)
    scratch = torch.empty(_lib.FUSION_WARPED_SCRATCH_BYTES // 8, dtype=torch.float64, device=tsdf.device)

    def ptr(t):
        return ctypes.c_void_p(None if t is None else t.data_ptr())

    check(lib.lsf_fusion_integrate_depth_warped(
        ptr(tsdf), ptr(weight), ptr(colour), ptr(warp), ptr(depth), ptr(pixel_weight), ptr(colour_image), ptr(record),
        ptr(scratch), ctypes.byref(p), stream_ptr()), "lsf_fusion_integrate_depth_warped")
    return record


def unpack_record(r):
    """the host record (RECORD float64) as a dict: exact counts as ints, the float64 sum and the max"""
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    return {"fused": int(r[0]), "first_seen": int(r[1]), "sum_abs_change": float(r[2]),
            "max_abs_change": float(r[3])}


def unpack_weighted_record(r):
    """unpack_record of a weighted call, with its two further exact counts: carved and weight_rejected"""
    out = unpack_record(r)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    out["carved"], out["weight_rejected"] = int(r[4]), int(r[5])
    return out


def unpack_colour_record(r):
    """unpack_weighted_record of a colour call, with its two further exact counts: coloured and first_coloured"""
    out = unpack_weighted_record(r)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    out["coloured"], out["first_coloured"] = int(r[6]), int(r[7])
    return out


def unpack_warped_record(r):
    """unpack_colour_record of a warped call (coloured and first_coloured are 0 without colour), with the exact count of
    voxels whose displacement was not finite: warp_rejected"""
    out = unpack_colour_record(r)
    out["warp_rejected"] = int(np.asarray(r, dtype=np.float64).reshape(-1)[8])
    return out
