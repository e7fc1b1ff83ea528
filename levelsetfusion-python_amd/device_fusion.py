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


def _check_tensor(name, t, dtype, device_name, device_like, shape_name, shape_like, extra, rule):
    """what every optional buffer of a call is checked for before its aliasing: a torch tensor of `dtype`, on
    device_like's device, contiguous, of shape_like's shape + extra; `rule` words the shape's refusal"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, str(dtype).split(".")[-1], t.dtype))
    if t.device != device_like.device:
        raise ValueError("%s is on %s, %s on %s: all buffers must be on one device"
                         % (name, t.device, device_name, device_like.device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if tuple(t.shape) != tuple(shape_like.shape) + extra:
        raise ValueError("%s has shape %s, %s %s: %s" % (name, tuple(t.shape), shape_name, tuple(shape_like.shape), rule))


def _check_others(name, t, others):
    for other, o in others:
        if o is not None and _overlap(t, o):
            raise ValueError("%s must not alias %s" % (name, other))


def check_pixel_weight(pixel_weight, depth, tsdf, weight):
    """a weight image: a float32 contiguous tensor on the model's device, of the depth image's shape, aliasing neither
    the model nor the depth image"""
    _check_tensor("pixel_weight", pixel_weight, torch.float32, "tsdf", tsdf, "the depth image", depth, (),
                  "they must have one shape")
    if _overlap(pixel_weight, tsdf) or _overlap(pixel_weight, weight) or _overlap(pixel_weight, depth):
        raise ValueError("pixel_weight must not alias tsdf, weight or the depth image")


def colour_band_of(colour_band):
    """colour_band as a float32 value after the rule's check: finite and in (0, 1]"""
    band = np.float32(colour_band)
    if not (band > 0 and band <= 1):  # NaN fails
        raise ValueError("colour_band must be finite and in (0, 1], got %r" % (colour_band,))
    return float(band)


def check_colour_volume(colour, tsdf, weight):
    """a colour volume: a float32 contiguous tensor of shape tsdf.shape + (4,) on the model's device, 16-byte aligned,
    aliasing neither tsdf nor weight"""
    _check_tensor("colour", colour, torch.float32, "tsdf", tsdf, "the model", tsdf, (4,),
                  "it must be the model's shape + (4,)")
    if colour.data_ptr() % 16:
        raise ValueError("colour must be 16-byte aligned: a voxel's record is one 16-byte access")
    if _overlap(colour, tsdf) or _overlap(colour, weight):
        raise ValueError("colour must not alias tsdf or weight")


def check_colour_image(colour_image, depth, others):
    """a colour image: a uint8 contiguous (H, W, 3) tensor on the depth image's device, H and W the depth image's,
    aliasing none of `others` ((name, tensor) pairs; None tensors are skipped)"""
    _check_tensor("colour_image", colour_image, torch.uint8, "the depth image", depth, "the depth image", depth, (3,),
                  "it must be (H, W, 3) with the depth image's H, W")
    _check_others("colour_image", colour_image, others)


def check_warp(warp, tsdf, others):
    """a warp field: a float32 contiguous tensor of shape tsdf.shape + (3,) on the model's device (what
    HierarchicalOptimizer3d.optimize returns for device inputs), aliasing none of `others` ((name, tensor) pairs; None
    tensors are skipped)"""
    _check_tensor("warp", warp, torch.float32, "tsdf", tsdf, "the model", tsdf, (3,),
                  "it must be the model's shape + (3,)")
    _check_others("warp", warp, others)


# the three entry points of the weighted rule: the C function, its parameter struct (lsf_fusion_weighted_params, and what
# is nested around it), its scratch bytes and its record's doubles
_WEIGHTED = ("lsf_fusion_integrate_depth_weighted", FusionWeightedParams, _lib.FUSION_WEIGHTED_SCRATCH_BYTES, RECORD)
_COLOUR = ("lsf_fusion_integrate_depth_colour", FusionColourParams, _lib.FUSION_COLOUR_SCRATCH_BYTES, RECORD)
_WARPED = ("lsf_fusion_integrate_depth_warped", FusionWarpedParams, _lib.FUSION_WARPED_SCRATCH_BYTES, WARPED_RECORD)


def _integrate_depth_weighted(entry, tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                              narrow_band_width_voxels, w, max_weight, pixel_weight, carve, record, colour=None,
                              colour_image=None, colour_band=1.0, warp=None):
    """the checks, the parameters and the call of one of the three: _COLOUR needs colour and colour_image, _WARPED takes
    them together or not at all and needs warp, _WEIGHTED takes none of the three"""
    name, params, scratch_bytes, doubles = entry
    require_gpu()
    if entry is _WARPED and (colour is None) != (colour_image is None):
        raise ValueError("colour and colour_image are given together or not at all")
    p = params()
    cp = p.colour if entry is _WARPED else p  # lsf_fusion_colour_params, where there is one
    wp = p if entry is _WEIGHTED else cp.weighted
    wp.fusion = _depth_params(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                              narrow_band_width_voxels, w, max_weight, 1)
    if pixel_weight is not None:
        check_pixel_weight(pixel_weight, depth, tsdf, weight)
    if entry is _COLOUR or colour is not None:
        check_colour_volume(colour, tsdf, weight)
        check_colour_image(colour_image, depth, (("tsdf", tsdf), ("weight", weight), ("colour", colour),
                                                 ("depth", depth), ("pixel_weight", pixel_weight)))
        if _overlap(colour, depth) or (pixel_weight is not None and _overlap(colour, pixel_weight)):
            raise ValueError("colour must not alias the depth image or pixel_weight")
    if entry is _WARPED:
        check_warp(warp, tsdf, (("tsdf", tsdf), ("weight", weight), ("colour", colour), ("depth", depth),
                                ("pixel_weight", pixel_weight), ("colour_image", colour_image)))
        p.has_colour = int(colour is not None)
    wp.carve, wp.has_pixel_weight = int(bool(carve)), int(pixel_weight is not None)
    ptr = ctypes.c_void_p
    pw = ptr(None if pixel_weight is None else pixel_weight.data_ptr())
    if entry is _WEIGHTED:
        between = (ptr(depth.data_ptr()), pw)
    else:  # colour, [warp,] depth, pixel_weight, colour_image
        cp.colour_band = colour_band_of(colour_band)
        between = (ptr(depth.data_ptr()), pw, ptr(None if colour_image is None else colour_image.data_ptr()))
        if entry is _WARPED:
            between = (ptr(warp.data_ptr()),) + between
        between = (ptr(None if colour is None else colour.data_ptr()),) + between
    if record is None:
        record = torch.empty(doubles, dtype=torch.float64, device=tsdf.device)
    scratch = torch.empty(scratch_bytes // 8, dtype=torch.float64, device=tsdf.device)
    check(getattr(lib, name)(ptr(tsdf.data_ptr()), ptr(weight.data_ptr()), *between, ptr(record.data_ptr()),
                             ptr(scratch.data_ptr()), ctypes.byref(p), stream_ptr()), name)
    return record


def integrate_depth_weighted(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                             narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None, carve=False,
                             record=None):
    """integrate_depth with the weighted rule ("Weighted fusion and carving"): a voxel's
    weight is w times pixel_weight at the pixel it projects to (a float32 device image of depth's shape; None: w
    itself), and with carve the seen free space in front of the band (live value exactly 1 at a valid pixel) is fused
    with +1.  Two launches, no host wait; returns the record (unpack_weighted_record once it is on the host)"""
    return _integrate_depth_weighted(_WEIGHTED, tsdf, weight, depth, depth_code, camera, array_offset, twist,
                                     voxel_size, narrow_band_width_voxels, w, max_weight, pixel_weight, carve, record)


def integrate_depth_colour(tsdf, weight, colour, depth, depth_code, camera, array_offset, twist, colour_image,
                           voxel_size=0.004, narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None,
                           carve=False, colour_band=1.0, record=None):
    """integrate_depth_weighted that also fuses colour_image (uint8 (H, W, 3) device tensor registered to the depth
    image) into the colour volume (float32, tsdf.shape + (4,): R, G, B in 0..255 and the colour weight) of the voxels
    whose live value lies strictly inside (-colour_band, colour_band) ("Colour fusion").
    tsdf, weight and record slots 0..5 are integrate_depth_weighted's bit for bit.  Two launches, no host wait; returns
    the record (unpack_colour_record once it is on the host)"""
    return _integrate_depth_weighted(_COLOUR, tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                                     narrow_band_width_voxels, w, max_weight, pixel_weight, carve, record, colour,
                                     colour_image, colour_band)


def integrate_depth_warped(tsdf, weight, depth, depth_code, camera, array_offset, twist, warp, voxel_size=0.004,
                           narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None, carve=False,
                           colour=None, colour_image=None, colour_band=1.0, record=None):
    """integrate_depth_weighted -- and integrate_depth_colour, when colour and colour_image are given (both or neither)
    -- through a non-rigid warp field ("Warped depth fusion"): warp is a float32 device tensor
    of shape tsdf.shape + (3,), channel 0 the x displacement, 1 y, 2 z, in voxels; voxel v observes the frame at
    v + warp[v] in place of its centre, and a voxel whose displacement is not finite is left alone and counted.  With a
    zero warp the result equals those calls bit for bit.  Two launches, no host wait; returns the record, WARPED_RECORD
    doubles (unpack_warped_record once it is on the host)"""
    return _integrate_depth_weighted(_WARPED, tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size,
                                     narrow_band_width_voxels, w, max_weight, pixel_weight, carve, record, colour,
                                     colour_image, colour_band, warp)


def integrate_depth_by_arguments(tsdf, weight, depth, depth_code, camera, array_offset, twist, voxel_size=0.004,
                                 narrow_band_width_voxels=20., w=1.0, max_weight=math.inf, pixel_weight=None, carve=False,
                                 colour=None, colour_image=None, colour_band=1.0, warp=None):
    """the depth-mode call that the arguments ask for: integrate_depth_warped with a warp, else integrate_depth_colour
    with a colour_image, else integrate_depth_weighted with a pixel_weight or carve, else integrate_depth.  `colour`,
    the model's colour volume, is used with a colour_image only.  Returns (record, unpack): the device record and the
    unpack_* function that reads a host copy of it"""
    gen = (voxel_size, narrow_band_width_voxels, w, max_weight)
    if warp is not None:
        coloured = colour_image is not None
        return integrate_depth_warped(tsdf, weight, depth, depth_code, camera, array_offset, twist, warp, *gen,
                                      pixel_weight, carve, colour if coloured else None, colour_image,
                                      colour_band), unpack_warped_record
    if colour_image is not None:
        return integrate_depth_colour(tsdf, weight, colour, depth, depth_code, camera, array_offset, twist,
                                      colour_image, *gen, pixel_weight, carve, colour_band), unpack_colour_record
    if pixel_weight is not None or carve:
        return integrate_depth_weighted(tsdf, weight, depth, depth_code, camera, array_offset, twist, *gen,
                                        pixel_weight, carve), unpack_weighted_record
    return integrate_depth(tsdf, weight, depth, depth_code, camera, array_offset, twist, *gen), unpack_record


def _unpack(r, fields):
    """the host record as a dict of `fields`: exact counts as ints, the float64 sum and the max as floats"""
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    return {f: (float if f in ("sum_abs_change", "max_abs_change") else int)(r[i]) for i, f in enumerate(fields)}


def unpack_record(r):
    """the host record (RECORD float64) as a dict: exact counts as ints, the float64 sum and the max"""
    return _unpack(r, RECORD_FIELDS)


def unpack_weighted_record(r):
    """unpack_record of a weighted call, with its two further exact counts: carved and weight_rejected"""
    return _unpack(r, WEIGHTED_RECORD_FIELDS)


def unpack_colour_record(r):
    """unpack_weighted_record of a colour call, with its two further exact counts: coloured and first_coloured"""
    return _unpack(r, COLOUR_RECORD_FIELDS)


def unpack_warped_record(r):
    """unpack_colour_record of a warped call (coloured and first_coloured are 0 without colour), with the exact count of
    voxels whose displacement was not finite: warp_rejected"""
    return _unpack(r, WARPED_RECORD_FIELDS)
