"""A verdict on every tracked frame and a way back when the track is lost ("Tracking quality
and relocalisation"; tests/relocaliser_restatement.py restates both).  TrackingQuality reads the last ICP record of a
frame -- the 64 doubles lsf_icp_run* and lsf_point_sdf_run* already write -- and is host arithmetic only.  Relocaliser
keeps keyframes encoded by random ferns (Glocker et al., "Real-time RGB-D camera relocalization via randomized ferns"):
the fern table is drawn on the host, the database of codes lives on the device (csrc/lsf_relocaliser.hip through
device_relocaliser), the keyframes' twists on the host.  SequenceFusion3d(tracking_quality=, relocaliser=) uses both."""
import math

import numpy as np
import torch

from .. import device_relocaliser
from ..device_core import require_gpu
from ..rigid_opt.frame_tracker import device_colour_image
from ..tsdf.generation import device_depth

TRACKING_STATES = ("tracking", "lost", "relocalised", "recovering")


class TrackingQuality:
    """the gate on a tracked frame.  A frame is good when its last record is not skipped, its pair fraction
    count * s^2 / (H * W) is at least min_pair_fraction (s the stride of the record's level; the fraction is over the
    image's pixels, valid or not) and its RMS residual sqrt(energy / count) is at most max_rms (metres; 0 for a record
    without pairs).  A frame without a record -- it ran no iteration -- is good."""

    def __init__(self, min_pair_fraction=0.25, max_rms=math.inf):
        self.min_pair_fraction, self.max_rms = float(min_pair_fraction), float(max_rms)
        if not (math.isfinite(self.min_pair_fraction) and 0 <= self.min_pair_fraction <= 1):
            raise ValueError("min_pair_fraction must lie in [0, 1], got %r" % (min_pair_fraction,))
        if math.isnan(self.max_rms) or self.max_rms < 0:
            raise ValueError("max_rms must be >= 0 (math.inf for no gate), got %r" % (max_rms,))

    def judge(self, record, image_shape, stride):
        """{good, pair_fraction, rms, skipped} of one unpacked ICP record (device_icp.unpack_record's dict; None for a
        frame without one), the frame's (H, W) and the stride of the record's level"""
        if record is None:
            return {"good": True, "pair_fraction": None, "rms": None, "skipped": False}
        count, skipped = int(record["count"]), bool(record["skipped"])
        fraction = count * float(stride) ** 2 / (float(image_shape[0]) * float(image_shape[1]))
        rms = math.sqrt(float(record["energy"]) / count) if count > 0 else 0.0
        good = not skipped and fraction >= self.min_pair_fraction and rms <= self.max_rms
        return {"good": bool(good), "pair_fraction": fraction, "rms": rms, "skipped": skipped}


def level_stride(tracker, level):
    """the stride of iteration level `level` of a FrameTracker (ProjectiveIcp3d, PointToSdf3d): its own stride on the
    strided path; on a pyramid 2^L of the pyramid level L = len(iterations) - 1 - level that the iterations' level uses"""
    if tracker.pyramid is None:
        return int(tracker.strides[level])
    return 2 ** (len(tracker.iterations) - 1 - int(level))


def fern_table(ferns, decisions, coarse_shape, depth_range, colour, seed):
    """(locations int32, channels uint8, thresholds float32), each (ferns, decisions), drawn from
    numpy.random.default_rng(seed) in this order: the locations, uniform over the coarse pixels; the channels, 0 (depth)
    without colour and uniform over 0..3 with it; one uniform per decision, scaled to depth_range for a depth decision
    and to [0, 255] for a colour decision"""
    rng = np.random.default_rng(seed)
    shape = (int(ferns), int(decisions))
    locations = rng.integers(0, int(coarse_shape[0]) * int(coarse_shape[1]), shape).astype(np.int32)
    channels = (rng.integers(0, 4, shape) if colour else np.zeros(shape)).astype(np.uint8)
    u = rng.random(shape)
    near, far = depth_range
    thresholds = np.where(channels == 0, near + u * (far - near), u * 255.0).astype(np.float32)
    return locations, channels, thresholds


class Relocaliser:
    """keyframes by random ferns.  ferns, decisions: the code is `ferns` bytes of `decisions` bits; coarse_shape: the
    (rows, columns) of the coarse image a frame is reduced to; depth_range: (near, far) in metres, the depths that count
    and the range of the depth thresholds; harvest_threshold: a frame becomes a keyframe when more than this fraction of
    its ferns differs from every keyframe's; max_keyframes: the database's rows; candidates: how many nearest keyframes
    a query returns (1..4); resume_after: how many good frames from a relocalisation on, the relocalised one included,
    SequenceFusion3d tracks without fusing; seed: of the fern table.  The table is drawn at the first encode, when the
    frame says whether there is colour (every later frame must agree); `codes` (uint8 (max_keyframes, ferns)) and
    `size` (int32 (1,)) are the device database, `twists` the keyframes' poses on the host."""

    def __init__(self, ferns=500, decisions=4, coarse_shape=(30, 40), depth_range=(0.2, 4.0), harvest_threshold=0.2,
                 max_keyframes=1024, candidates=1, resume_after=0, seed=0):
        R = device_relocaliser
        # the checks of a query with these settings, made now: a host error at construction, not at the first frame
        p = R.query_params(coarse_shape, 1, ferns, decisions, max_keyframes, candidates)
        self.ferns, self.decisions, self.max_keyframes, self.candidates = p.ferns, p.decisions, p.capacity, p.candidates
        self.coarse_shape = (p.coarse_height, p.coarse_width)
        self.depth_range = R.depth_range_of(depth_range)
        self.harvest_threshold = float(harvest_threshold)
        self.harvest_differing = R.harvest_differing_of(harvest_threshold, self.ferns)
        self.resume_after = int(resume_after)
        if self.resume_after != resume_after or self.resume_after < 0:
            raise ValueError("resume_after must be a whole number >= 0, got %r" % (resume_after,))
        self.seed = seed
        np.random.default_rng(seed)  # a seed numpy refuses is refused here
        self.colour = None  # decided by the first frame
        self.table = None   # the host (locations, channels, thresholds)
        self.twists = []
        self._device = None

    def _prepare(self, colour):
        if self.colour is None:
            self.colour = bool(colour)
            self.table = fern_table(self.ferns, self.decisions, self.coarse_shape, self.depth_range, self.colour,
                                    self.seed)
        elif self.colour != bool(colour):
            raise ValueError("this relocaliser's fern table was drawn %s colour; every frame must come the same way"
                             % ("with" if self.colour else "without"))
        if self._device is None:
            require_gpu()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
            self._device = tuple(up(a) for a in self.table)
            self.codes = torch.zeros((self.max_keyframes, self.ferns), dtype=torch.uint8, device="cuda")
            self.size = torch.zeros(1, dtype=torch.int32, device="cuda")

    def encode(self, depth_image, camera=None, colour_image=None, depth_unit_ratio=None):
        """the coarse image of a frame (depth uint16 / float32 / float64, numpy or device; colour uint8 (H, W, 3) or
        None), a float32 (rows, columns, C) device tensor; `last_encode_record` keeps the call's device record.  The
        depth is scaled by camera.depth_unit_ratio, or by depth_unit_ratio when given"""
        depth, _ = device_depth(depth_image)
        if depth_unit_ratio is None:
            depth_unit_ratio = 1.0 if camera is None else camera.depth_unit_ratio
        colour = None if colour_image is None else device_colour_image(colour_image)
        self._prepare(colour is not None)
        coarse, _, self.last_encode_record = device_relocaliser.encode(depth, self.coarse_shape, self.depth_range,
                                                                       depth_unit_ratio, colour)
        return coarse

    def query(self, coarse, harvest=False, twist=None):
        """lsf_reloc_query of a coarse image against the database, and the one host copy of its record.  Returns
        device_relocaliser.unpack_query_record's dict.  With harvest the frame is appended when the rule wants it and
        there is room, and `twist` -- required then -- becomes that keyframe's pose"""
        if self._device is None:
            raise ValueError("encode a frame first: the fern table is drawn when the first frame says whether there is "
                             "colour")
        if harvest and twist is None:
            raise ValueError("a harvesting query needs the frame's twist")
        _, self.last_distances, record = device_relocaliser.query(
            coarse, *self._device, self.codes, self.size, self.candidates, harvest, self.harvest_differing)
        out = device_relocaliser.unpack_query_record(record.cpu().numpy())
        if out["appended"] is not None:
            assert out["appended"] == len(self.twists)
            self.twists.append(np.asarray(twist, dtype=np.float64).reshape(6).copy())
        return out

    def keyframes(self):
        """(codes uint8 (n, ferns), twists float64 (n, 6)): host copies of the database"""
        n = len(self.twists)
        codes = np.zeros((0, self.ferns), np.uint8) if self._device is None else self.codes[:n].cpu().numpy()
        return codes, np.array(self.twists, dtype=np.float64).reshape(n, 6)

    def reset(self):
        """forget every keyframe; the fern table stays"""
        self.twists = []
        if self._device is not None:
            self.size.zero_()
