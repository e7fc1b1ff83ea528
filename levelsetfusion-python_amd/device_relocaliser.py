"""Torch-facing wrappers of the keyframe ferns on the card (include/lsf_hip.h: lsf_reloc_encode, lsf_reloc_query;
INTEGRATION.md section 3, "Tracking quality and relocalisation"; tests/relocaliser_restatement.py restates them), and the
host rules of their arguments.  Every argument is checked on the host before a launch; workspaces are torch tensors; the
calls are enqueued and nothing waits.  The public interface is fusion.Relocaliser and
fusion.SequenceFusion3d(relocaliser=)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import RelocParams, check, lib
from .device_core import require_gpu, stream_ptr
from .device_rgbd import _check_buffer, _no_alias, _ptr

MAX_FERNS = _lib.RELOC_MAX_FERNS
MAX_DECISIONS = _lib.RELOC_MAX_DECISIONS
MAX_CANDIDATES = _lib.RELOC_MAX_CANDIDATES
MAX_DEPTH = _lib.RELOC_MAX_DEPTH
ENCODE_RECORD_FIELDS = ("counting", "valid_blocks")
QUERY_RECORD_WORDS = _lib.RELOC_QUERY_RECORD_WORDS
INT32_MAX = 2 ** 31 - 1
_DEPTH_CODES = {torch.uint16: _lib.DEPTH_U16, torch.float32: _lib.DEPTH_F32, torch.float64: _lib.DEPTH_F64}


def _whole(value, name, lo, hi):
    v = int(value)
    if v != value or not lo <= v <= hi:
        raise ValueError("%s must be a whole number in [%d, %d], got %r" % (name, lo, hi, value))
    return v


def coarse_shape_of(coarse_shape):
    """(coarse_height, coarse_width), whole numbers >= 1 whose product fits an int32 with four channels"""
    if np.ndim(coarse_shape) != 1 or len(coarse_shape) != 2:
        raise ValueError("coarse_shape must be (rows, columns), got %r" % (coarse_shape,))
    ch, cw = (_whole(v, "coarse_shape", 1, INT32_MAX) for v in coarse_shape)
    if ch * cw * 4 > INT32_MAX:
        raise ValueError("a coarse image of %d x %d has more values than int32 indices reach" % (ch, cw))
    return ch, cw


def depth_range_of(depth_range):
    """(near, far) in metres as floats: finite, 0 < near < far <= MAX_DEPTH"""
    if np.ndim(depth_range) != 1 or len(depth_range) != 2:
        raise ValueError("depth_range must be (near, far), got %r" % (depth_range,))
    near, far = float(depth_range[0]), float(depth_range[1])
    if not (math.isfinite(near) and math.isfinite(far) and 0 < near < far <= MAX_DEPTH):
        raise ValueError("depth_range needs 0 < near < far <= %g metres, got %r" % (MAX_DEPTH, depth_range))
    return near, far


def harvest_differing_of(harvest_threshold, ferns):
    """the least distance that appends a frame: floor(harvest_threshold * F) + 1, i.e. a fraction of differing ferns
    strictly above the threshold; the threshold is finite and in [0, 1)"""
    t = float(harvest_threshold)
    if not (math.isfinite(t) and 0 <= t < 1):
        raise ValueError("harvest_threshold must lie in [0, 1), got %r" % (harvest_threshold,))
    return int(math.floor(t * ferns)) + 1


def encode_params(shape, coarse_shape, depth_range, depth_unit_ratio=1.0, colour=False):
    """the lsf_reloc_params of lsf_reloc_encode after the host checks"""
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError("the frame needs extents (height, width) >= 1, got %s" % (tuple(shape),))
    p = RelocParams()
    p.height, p.width = int(shape[0]), int(shape[1])
    if p.height * p.width > INT32_MAX:
        raise ValueError("a frame of %d x %d has more pixels than int32 indices reach" % (p.height, p.width))
    p.coarse_height, p.coarse_width = coarse_shape_of(coarse_shape)
    if p.coarse_height > p.height or p.coarse_width > p.width:
        raise ValueError("the coarse image (%d x %d) must not exceed the frame (%d x %d): every block needs a pixel"
                         % (p.coarse_height, p.coarse_width, p.height, p.width))
    p.depth_near, p.depth_far = depth_range_of(depth_range)
    ratio = float(depth_unit_ratio)
    if not (math.isfinite(ratio) and ratio > 0):
        raise ValueError("depth_unit_ratio must be finite and > 0, got %r" % (depth_unit_ratio,))
    p.depth_unit_ratio = ratio
    p.channels = 4 if colour else 1
    return p


def query_params(coarse_shape, channels, ferns, decisions, capacity, candidates=1, harvest=False,
                 harvest_differing=1):
    """the lsf_reloc_params of lsf_reloc_query after the host checks"""
    p = RelocParams()
    p.coarse_height, p.coarse_width = coarse_shape_of(coarse_shape)
    if channels not in (1, 4):
        raise ValueError("a coarse image has 1 channel (depth) or 4 (depth, R, G, B), got %r" % (channels,))
    p.channels = int(channels)
    p.ferns = _whole(ferns, "ferns", 1, MAX_FERNS)
    p.decisions = _whole(decisions, "decisions", 1, MAX_DECISIONS)
    p.capacity = _whole(capacity, "capacity", 1, INT32_MAX)
    if p.capacity * p.ferns > INT32_MAX:
        raise ValueError("a database of %d keyframes of %d ferns has more bytes than int32 indices reach"
                         % (p.capacity, p.ferns))
    p.candidates = _whole(candidates, "candidates", 1, MAX_CANDIDATES)
    p.harvest = 1 if harvest else 0
    p.harvest_differing = _whole(harvest_differing, "harvest_differing", 1, INT32_MAX) if harvest else 0
    return p


def encode(depth, coarse_shape, depth_range, depth_unit_ratio=1.0, colour=None, coarse=None, block_counts=None,
           record=None):
    """lsf_reloc_encode: the device depth image (uint16 / float32 / float64, (H, W)) and, optionally, its registered
    uint8 (H, W, 3) colour image reduced to the coarse image of block means.  Returns (coarse float32 (ch, cw, C) with
    C = 1 or 4, block_counts int32 (ch, cw), record int32 (2,): ENCODE_RECORD_FIELDS), on the device.  Two launches,
    enqueued; nothing waits"""
    require_gpu()
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.dtype not in _DEPTH_CODES:
        raise ValueError("depth must be a 2-D uint16, float32 or float64 device tensor (tsdf.generation.device_depth)")
    _check_buffer("depth", depth, None, None, aligned=depth.element_size())
    p = encode_params(tuple(depth.shape), coarse_shape, depth_range, depth_unit_ratio, colour is not None)
    dev = depth.device
    if colour is not None:
        _check_buffer("colour", colour, torch.uint8, (p.height, p.width, 3), dev)
    ch, cw, c = p.coarse_height, p.coarse_width, p.channels
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    coarse = new((ch, cw, c), torch.float32) if coarse is None else coarse
    block_counts = new((ch, cw), torch.int32) if block_counts is None else block_counts
    record = new((len(ENCODE_RECORD_FIELDS),), torch.int32) if record is None else record
    _check_buffer("coarse", coarse, torch.float32, (ch, cw, c), dev, aligned=4)
    _check_buffer("block_counts", block_counts, torch.int32, (ch, cw), dev, aligned=4)
    _check_buffer("record", record, torch.int32, (len(ENCODE_RECORD_FIELDS),), dev, aligned=4)
    _no_alias([("depth", depth), ("colour", colour), ("coarse", coarse), ("block_counts", block_counts),
               ("record", record)])
    check(lib.lsf_reloc_encode(_ptr(depth), _DEPTH_CODES[depth.dtype], _ptr(colour), _ptr(coarse), _ptr(block_counts),
                               _ptr(record), ctypes.byref(p), stream_ptr()), "lsf_reloc_encode")
    return coarse, block_counts, record


def query(coarse, locations, channels, thresholds, codes, n_keyframes, candidates=1, harvest=False,
          harvest_differing=1, frame_code=None, distances=None, record=None):
    """lsf_reloc_query: the coarse image (ch, cw, C) against the fern table (locations int32, channels uint8,
    thresholds float32, each (F, D)) and the database (codes uint8 (capacity, F), 16-byte aligned; n_keyframes int32
    (1,)), all on the device.  Returns (frame_code uint8 (F,), distances int32 (capacity,), record int32 (12,)); with
    harvest the database may grow by the frame (codes and n_keyframes are written).  Three launches, enqueued"""
    require_gpu()
    if not isinstance(coarse, torch.Tensor) or coarse.dim() != 3:
        raise ValueError("coarse must be a float32 (rows, columns, channels) device tensor")
    if not isinstance(locations, torch.Tensor) or locations.dim() != 2:
        raise ValueError("locations must be an int32 (ferns, decisions) device tensor")
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2:
        raise ValueError("codes must be a uint8 (capacity, ferns) device tensor")
    f, d = (int(v) for v in locations.shape)
    p = query_params(tuple(coarse.shape[:2]), int(coarse.shape[2]), f, d, int(codes.shape[0]), candidates, harvest,
                     harvest_differing)
    dev = coarse.device
    _check_buffer("coarse", coarse, torch.float32, None, aligned=4)
    _check_buffer("locations", locations, torch.int32, (f, d), dev, aligned=4)
    _check_buffer("channels", channels, torch.uint8, (f, d), dev)
    _check_buffer("thresholds", thresholds, torch.float32, (f, d), dev, aligned=4)
    _check_buffer("codes", codes, torch.uint8, (p.capacity, f), dev, aligned=16)
    _check_buffer("n_keyframes", n_keyframes, torch.int32, (1,), dev, aligned=4)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    frame_code = new((f,), torch.uint8) if frame_code is None else frame_code
    distances = new((p.capacity,), torch.int32) if distances is None else distances
    record = new((QUERY_RECORD_WORDS,), torch.int32) if record is None else record
    _check_buffer("frame_code", frame_code, torch.uint8, (f,), dev)
    _check_buffer("distances", distances, torch.int32, (p.capacity,), dev, aligned=4)
    _check_buffer("record", record, torch.int32, (QUERY_RECORD_WORDS,), dev, aligned=4)
    _no_alias([("coarse", coarse), ("locations", locations), ("channels", channels), ("thresholds", thresholds),
               ("codes", codes), ("n_keyframes", n_keyframes), ("frame_code", frame_code), ("distances", distances),
               ("record", record)])
    check(lib.lsf_reloc_query(_ptr(coarse), _ptr(locations), _ptr(channels), _ptr(thresholds), _ptr(codes),
                              _ptr(n_keyframes), _ptr(frame_code), _ptr(distances), _ptr(record), ctypes.byref(p),
                              stream_ptr()), "lsf_reloc_query")
    return frame_code, distances, record


def unpack_encode_record(record):
    """{counting, valid_blocks} of a host copy of lsf_reloc_encode's record"""
    r = np.asarray(record).reshape(-1)
    return {name: int(r[i]) for i, name in enumerate(ENCODE_RECORD_FIELDS)}


def unpack_query_record(record):
    """{n, nearest, distances, appended, full} of a host copy of lsf_reloc_query's record: nearest and distances list
    the keyframes found, nearest first (shorter than `candidates` when the database is smaller); appended is the new
    keyframe's id or None; full says that a frame the harvest rule wanted met a full database"""
    r = np.asarray(record).reshape(-1)
    ids = [int(v) for v in r[1:1 + MAX_CANDIDATES] if v >= 0]
    return {"n": int(r[0]), "nearest": ids, "distances": [int(v) for v in r[5:5 + len(ids)]],
            "appended": None if r[9] < 0 else int(r[9]), "full": bool(r[10])}
