"""Numpy restatements of tracking quality and relocalisation ("Tracking quality and
relocalisation"), which the HIP kernels (lsf_reloc_encode / lsf_reloc_query in csrc/lsf_relocaliser.hip), the package's
host rules (fusion.TrackingQuality, fusion.Relocaliser's fern table) and SequenceFusion3d's state machine must equal.
Written from the contract: blocks are slices of the image, sums are numpy integer sums, the nearest keyframes come from a
lexicographic sort.  The sequence is restated on top of icp_restatement, raycast_restatement and fusion_restatement.
Host numpy only: no package import."""
import math

import numpy as np

import fusion_restatement as F
import icp_restatement as I
import raycast_restatement as RC

QUANTUM = 2.0 ** 20
MAX_CANDIDATES = 4


def scaled_depth(depth, ratio):
    """the depth in metres as float64, scaled as the generators scale it: float32 in float32, uint16 and float64 in
    float64"""
    d = np.asarray(depth)
    if d.dtype == np.float32:
        return (d * np.float32(ratio)).astype(np.float64)
    return d.astype(np.float64) * float(ratio)


def encode(depth, ratio, coarse_shape, depth_range, colour=None):
    """(coarse float32 (ch, cw, C), block_counts int32 (ch, cw), record {counting, valid_blocks}); C is 1 without and 4
    with a colour image"""
    d = scaled_depth(depth, ratio)
    h, w = d.shape
    ch, cw = coarse_shape
    near, far = depth_range
    with np.errstate(invalid="ignore"):
        counts = (d >= near) & (d <= far)
    q = np.rint(d * QUANTUM)
    q = np.where(counts, q, 0.0).astype(np.int64)
    coarse = np.zeros((ch, cw, 1 if colour is None else 4), np.float32)
    block_counts = np.zeros((ch, cw), np.int32)
    for i in range(ch):
        rows = slice(i * h // ch, (i + 1) * h // ch)
        for j in range(cw):
            cols = slice(j * w // cw, (j + 1) * w // cw)
            m = counts[rows, cols]
            n = int(m.sum())
            block_counts[i, j] = n
            if 2 * n < m.size:
                continue
            coarse[i, j, 0] = np.float32(float(q[rows, cols].sum()) / float(n) / QUANTUM)
            if colour is not None:
                for c in range(3):
                    total = int(np.asarray(colour)[rows, cols, c].astype(np.int64)[m].sum())
                    coarse[i, j, 1 + c] = np.float32(float(total) / float(n))
    record = {"counting": int(block_counts.sum()), "valid_blocks": int((coarse[..., 0] > 0).sum())}
    return coarse, block_counts, record


def fern_table(ferns, decisions, coarse_shape, depth_range, colour, seed):
    """fusion.relocaliser.fern_table's draw, restated: locations, then channels (with colour), then one uniform per
    decision"""
    rng = np.random.default_rng(seed)
    shape = (ferns, decisions)
    locations = rng.integers(0, coarse_shape[0] * coarse_shape[1], shape).astype(np.int32)
    channels = (rng.integers(0, 4, shape) if colour else np.zeros(shape)).astype(np.uint8)
    u = rng.random(shape)
    thresholds = np.where(channels == 0, depth_range[0] + u * (depth_range[1] - depth_range[0]),
                          u * 255.0).astype(np.float32)
    return locations, channels, thresholds


def frame_code(coarse, locations, channels, thresholds):
    """uint8 (F,): bit j of fern f is set when the coarse value at its location and channel exceeds the threshold and
    the block has a depth"""
    flat = coarse.reshape(-1, coarse.shape[2])
    code = np.zeros(locations.shape[0], np.uint8)
    for j in range(locations.shape[1]):
        loc, c = locations[:, j].astype(np.int64), channels[:, j].astype(np.int64)
        inside = (loc >= 0) & (loc < len(flat)) & (c < flat.shape[1])
        loc, c = np.where(inside, loc, 0), np.where(inside, c, 0)
        bit = inside & (flat[loc, c] > thresholds[:, j]) & (flat[loc, 0] > 0)
        code |= (bit.astype(np.uint8) << j).astype(np.uint8)
    return code


def harvest_differing(harvest_threshold, ferns):
    return int(math.floor(harvest_threshold * ferns)) + 1


def query(coarse, table, codes, n, candidates=1, harvest=False, differing=1):
    """lsf_reloc_query on host arrays: codes uint8 (capacity, F) and n are the database.  Returns (frame_code,
    distances int32 (capacity,), record int32 (12,), codes after, n after)"""
    capacity = codes.shape[0]
    code = frame_code(coarse, *table)
    n = min(max(int(n), 0), capacity)
    distances = np.full(capacity, -1, np.int32)
    distances[:n] = (codes[:n] != code[None, :]).sum(axis=1)
    order = sorted(range(n), key=lambda k: (int(distances[k]), k))[:candidates]
    record = np.zeros(12, np.int32)
    record[0] = n
    record[1:9] = -1
    for slot, k in enumerate(order):
        record[1 + slot], record[5 + slot] = k, distances[k]
    wanted = bool(harvest) and (n == 0 or int(distances[order[0]]) >= differing)
    record[9] = n if wanted and n < capacity else -1
    record[10] = 1 if wanted and n >= capacity else 0
    codes = codes.copy()
    if record[9] >= 0:
        codes[n] = code
        n += 1
    return code, distances, record, codes, n


def judge(record, image_shape, stride, min_pair_fraction=0.25, max_rms=math.inf):
    """fusion.TrackingQuality.judge on an icp_restatement record (None: a frame that ran no iteration)"""
    if record is None:
        return {"good": True, "pair_fraction": None, "rms": None, "skipped": False}
    count, skipped = int(record["count"]), bool(record["skipped"])
    fraction = count * float(stride) ** 2 / (float(image_shape[0]) * float(image_shape[1]))
    rms = math.sqrt(float(record["energy"]) / count) if count > 0 else 0.0
    return {"good": (not skipped) and fraction >= min_pair_fraction and rms <= max_rms, "pair_fraction": fraction,
            "rms": rms, "skipped": skipped}


class Database:
    """fusion.Relocaliser on the host: the table, the codes, the twists"""

    def __init__(self, ferns=500, decisions=4, coarse_shape=(30, 40), depth_range=(0.2, 4.0), harvest_threshold=0.2,
                 max_keyframes=1024, candidates=1, resume_after=0, seed=0, colour=False):
        self.coarse_shape, self.depth_range = coarse_shape, depth_range
        self.table = fern_table(ferns, decisions, coarse_shape, depth_range, colour, seed)
        self.codes, self.n, self.twists = np.zeros((max_keyframes, ferns), np.uint8), 0, []
        self.candidates, self.resume_after = candidates, resume_after
        self.differing = harvest_differing(harvest_threshold, ferns)

    def encode(self, depth, ratio, colour=None):
        return encode(depth, ratio, self.coarse_shape, self.depth_range, colour)[0]

    def query(self, coarse, harvest=False, twist=None):
        _, distances, record, self.codes, self.n = query(coarse, self.table, self.codes, self.n, self.candidates,
                                                         harvest, self.differing)
        ids = [int(v) for v in record[1:5] if v >= 0]
        if record[9] >= 0:
            self.twists.append(np.array(twist, np.float64))
        return {"nearest": ids, "distances": [int(distances[k]) for k in ids],
                "appended": None if record[9] < 0 else int(record[9])}


def sequence(frames, K, ratio, shape, offset, quality=None, database=None, iterations=I.ITERATIONS, strides=I.STRIDES,
             max_distance=I.MAX_DISTANCE, band=20, voxel_size=0.004):
    """SequenceFusion3d(tracking_reference="icp", tracking_quality=, relocaliser=) without a non-rigid step, on top of
    icp_restatement.sequence's steps.  quality: None or (min_pair_fraction, max_rms); database: None or a Database (it
    implies quality (0.25, inf) when none is given).  Returns (tsdf, weight, twists, frame dicts: state, quality, fused,
    keyframe, relocalisation)."""
    if database is not None and quality is None:
        quality = (0.25, math.inf)
    tsdf, weight = F.empty_model(shape)
    twists, out = [], []
    state, recovering = "tracking", 0

    def attempt(depth, start):
        pd, pn, _ = RC.raycast(tsdf, weight, K, start, offset, voxel_size, np.shape(depth), normals=True)
        recs, twist = I.icp(depth, pd, pn, K, ratio, start, start, iterations, strides, max_distance)
        last = recs[-1] if recs else None
        return twist, judge(last, np.shape(depth), 1 if last is None else strides[last["level"]], *quality)

    for k, depth in enumerate(frames):
        frame = {"state": "tracking", "quality": None, "relocalisation": None, "keyframe": None}
        coarse = None if database is None else database.encode(depth, ratio)
        fuse = True
        if k == 0:
            twist = np.zeros(6)
        elif quality is None:
            pd, pn, _ = RC.raycast(tsdf, weight, K, twists[-1], offset, voxel_size, np.shape(depth), normals=True)
            _, twist = I.icp(depth, pd, pn, K, ratio, twists[-1], twists[-1], iterations, strides, max_distance)
        else:
            last_good = twists[-1]
            was_lost = database is not None and state == "lost"
            now, verdict = "lost", None
            if not was_lost:
                twist, verdict = attempt(depth, last_good)
                now = "tracking" if verdict["good"] else "lost"
            if now == "lost" and database is not None:
                found = database.query(coarse)
                frame["relocalisation"] = {"candidates": found["nearest"], "distances": found["distances"],
                                           "chosen": None}
                starts = [(i, database.twists[i]) for i in found["nearest"]] + ([(-1, last_good)] if was_lost else [])
                for chosen, start in starts:
                    twist, verdict = attempt(depth, start)
                    if verdict["good"]:
                        now, recovering = "relocalised", database.resume_after
                        frame["relocalisation"]["chosen"] = chosen
                        break
            good = now != "lost"
            fuse = good
            if good and recovering > 0:
                recovering -= 1
                fuse = False
                now = now if now == "relocalised" else "recovering"
            if not good:
                twist = last_good
            state = now
            frame["state"], frame["quality"] = now, verdict
        twist = np.array(twist, np.float64)
        if fuse:
            tsdf, weight, _ = F.fuse_depth(tsdf, weight, depth, K, ratio, offset, twist, band, voxel_size)
            if database is not None:
                frame["keyframe"] = database.query(coarse, harvest=True, twist=twist)["appended"]
        frame["fused"] = fuse
        twists.append(twist)
        out.append(frame)
    return tsdf, weight, twists, out
