"""Closed-form volumes and cameras at the edges of the ray-caster (csrc/lsf_raycast.hip) that a fused sphere scene never
reaches: rays that graze a face of the box with b_j == 0, cameras inside and behind the volume, rotations near and
beyond 90 degrees on a volume of three different extents, holes of unusable weight in front of the surface, samples
that are exactly 0, hits whose normal samples touch a hole or the border, colour weights with their own holes, a needle
of hundreds of steps along each axis, and images one off the wave block and the tile.  tests/test_raycast_edges_host.py
checks that each scene does what it claims; tests/test_gpu_raycast_edges.py runs the kernel on them.  Host numpy
only."""
import numpy as np

import raycast_restatement as RC

VOXEL = 0.25


class Case:
    """one ray-cast: a (Z, Y, X) model, a camera and an image shape"""

    def __init__(self, name, tsdf, weight, K, twist, offset, image_shape, colour=None):
        self.name, self.tsdf, self.weight, self.colour = name, tsdf, weight, colour
        self.K, self.twist, self.offset, self.image_shape = K, np.asarray(twist, np.float64), offset, image_shape
        self.voxel_size = VOXEL

    @property
    def step_cap(self):
        """the kernel's bound on a lane's steps past its first, 4 (X + Y + Z) + 8"""
        return 4 * sum(self.tsdf.shape) + 8

    def args(self):
        return self.tsdf, self.weight, self.K, self.twist, self.offset, self.voxel_size, self.image_shape

    def __repr__(self):
        return self.name


def _intrinsics(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float32)


# ---- ball: a sphere of radius 2.4 voxels about (5.3, 3.1, 4.2) in a (9, 7, 12) volume, truncated at 2 voxels
BALL_SHAPE = (9, 7, 12)
BALL_OFFSET = np.array([-5.5, -3.0, 6.0])
BALL_K = _intrinsics(30.0, 16.0, 10.0)
BALL_IMAGE = (21, 33)
BALL_CAMERAS = {  # name: (rotation vector, distance to the box centre along the optical axis)
    "front": ((0.0, 0.0, 0.0), 2.5),
    "behind": ((0.0, 0.0, 0.0), -3.0),
    "rx": ((0.9, 0.0, 0.0), 2.0),
    "ry": ((0.0, -1.1, 0.0), 2.2),
    "rz": ((0.0, 0.0, 2.0), 2.5),
    "back": ((0.0, 3.0, 0.0), 2.5),
    "mixed": ((0.5, -0.7, 0.4), 1.4),
}


def ball_tsdf():
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in BALL_SHAPE), indexing="ij")
    r = np.sqrt((x - 5.3) ** 2 + (y - 3.1) ** 2 + (z - 4.2) ** 2)
    return np.clip((r - 2.4) / 2.0, -1.0, 1.0).astype(np.float32)


def ball_weight(kind):
    w = np.ones(BALL_SHAPE, np.float32)
    if kind == "holes":
        w[2] = 0.0
        w[:, 3, 7] = np.nan
        w[6, 1, :] = -1.0
    elif kind != "ones":
        raise ValueError(kind)
    return w


def look_at(rotation, centre_world, dist):
    """the twist of a camera with this rotation vector whose optical axis passes through centre_world at camera depth
    dist: t = (0, 0, dist) - R centre"""
    r = np.asarray(rotation, np.float64)
    R = RC.extrinsic(np.concatenate([np.zeros(3), r]))[:, :3]
    t = np.array([0.0, 0.0, dist]) - R @ np.asarray(centre_world, np.float64)
    return np.concatenate([t, r])


def ball_twist(camera):
    rotation, dist = BALL_CAMERAS[camera]
    centre = (np.array([5.5, 3.0, 4.0]) + BALL_OFFSET) * VOXEL
    return look_at(rotation, centre, dist)


def ball(camera, weights="ones", image_shape=BALL_IMAGE, K=BALL_K, tsdf=None, colour=None, name=None):
    return Case(name or "ball/%s/%s" % (weights, camera), ball_tsdf() if tsdf is None else tsdf, ball_weight(weights), K,
                ball_twist(camera), BALL_OFFSET, image_shape, colour)


def ball_cases():
    return [ball(c, k) for k in ("ones", "holes") for c in BALL_CAMERAS]


# ---- slab: the plane z = 4 (z = 0.25 in entry-hit) seen along +z; the pixel column u = 8 runs along x = ax with b_x == 0 exactly
SLAB_SHAPE = (9, 6, 10)
SLAB_K = _intrinsics(32.0, 8.0, 4.0)
SLAB_IMAGE = (9, 17)
SLAB_CASES = {  # name: (ax, first z layer of positive weight, t_z in voxels, z of the surface)
    "graze-low": (0, 0, 2.0, 4.0),
    "graze-high": (9, 0, 2.0, 4.0),
    "mid": (4, 0, 2.0, 4.0),
    "exact-zero": (4, 3, 2.0, 4.0),
    "first-valid-zero": (4, 4, 2.0, 4.0),
    "inside": (4, 0, -1.25, 4.0),
    # the hit is every ray's second sample inside the box, and the sample before it lies exactly on the entry face
    # (lo / step is the integer 4): a lane that starts one step late has no previous sample and misses
    "entry-hit": (4, 0, 2.0, 0.25),
}


def slab(name):
    ax, first, tz, surface = SLAB_CASES[name]
    z = np.arange(SLAB_SHAPE[0], dtype=np.float32)[:, None, None]
    tsdf = np.broadcast_to((np.float32(surface) - z) / np.float32(4), SLAB_SHAPE).copy()
    weight = np.ones(SLAB_SHAPE, np.float32)
    weight[:first] = 0.0
    twist = np.array([-ax * VOXEL, -2.5 * VOXEL, tz * VOXEL, 0.0, 0.0, 0.0])
    return Case("slab/" + name, tsdf, weight, SLAB_K, twist, np.zeros(3), SLAB_IMAGE)


def slab_cases():
    return [slab(n) for n in SLAB_CASES]


# ---- needle: 120 voxels long and 2 x 2 across, the surface at index 100, the camera on the axis 3 voxels before
# index 0; a ray takes more than 200 steps to its hit.  The two transposes turn the long axis to x and to y, with the
# camera a float32 quarter turn about y and about x: its b_j across the needle are tiny and not 0
NEEDLE_K = _intrinsics(2000.0, 4.0, 4.0)
NEEDLE_IMAGE = (9, 9)
_QUARTER = float(np.float32(np.pi / 2))
NEEDLE_AXES = {  # long axis: (shape, axes of the base (Z, Y, X) array, rotation vector, camera centre in voxels)
    "z": ((120, 2, 2), (0, 1, 2), (0.0, 0.0, 0.0), (0.5, 0.5, -3.0)),
    "x": ((2, 2, 120), (2, 1, 0), (0.0, -_QUARTER, 0.0), (-3.0, 0.5, 0.5)),
    "y": ((2, 120, 2), (1, 0, 2), (_QUARTER, 0.0, 0.0), (0.5, -3.0, 0.5)),
}


def needle(axis):
    shape, axes, rotation, centre = NEEDLE_AXES[axis]
    z = np.arange(120, dtype=np.float64)[:, None, None]
    base = np.broadcast_to(np.clip((100.0 - z) / 4.0, -1.0, 1.0), (120, 2, 2)).astype(np.float32)
    tsdf = np.ascontiguousarray(np.transpose(base, axes))
    assert tsdf.shape == shape
    twist = look_at(rotation, np.asarray(centre) * VOXEL, 0.0)
    return Case("needle/" + axis, tsdf, np.ones(shape, np.float32), NEEDLE_K, twist, np.zeros(3), NEEDLE_IMAGE)


def needle_cases():
    return [needle(a) for a in NEEDLE_AXES]


# ---- crops: ball / ones / mixed at image shapes around the 8 x 8 wave block and the 16 x 16 tile; with one K each is
# the top-left crop of the 21 x 33 image
CROP_SHAPES = [(1, 1), (1, 17), (17, 1), (7, 9), (8, 8), (9, 7), (15, 17), (16, 16), (17, 15)]


def crop_cases():
    return [ball("mixed", "ones", s, name="crops/%dx%d" % s) for s in CROP_SHAPES]


# ---- colour: ball / holes with a colour volume whose weights have holes of their own
COLOUR_CAMERAS = ("front", "rx", "ry", "back", "mixed")


def colour_volume():
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in BALL_SHAPE), indexing="ij")
    c = np.empty(BALL_SHAPE + (4,), np.float32)
    c[..., 0] = 40.0 + 11.0 * x + 3.0 * y * z
    c[..., 1] = 230.0 - 17.0 * y - 2.0 * z * z
    c[..., 2] = 15.0 + 9.0 * z + 1.5 * x * y + 0.25 * x * x
    wc = np.ones(BALL_SHAPE, np.float32)
    wc[:, 5, :] = 0.0  # two planes, a row and two voxels the geometric weights keep
    wc[:, :, 2] = 0.0
    wc[5, 4, :] = 0.0
    wc[4, 3, 3] = np.nan
    wc[4, 2, 8] = -1.0
    c[..., 3] = wc
    return c


def colour_cases():
    return [ball(c, "holes", colour=colour_volume(), name="colour/" + c) for c in COLOUR_CAMERAS]


# ---- nonfinite: a NaN and a +inf tsdf under a positive weight
def nonfinite_cases():
    t = ball_tsdf()
    t[4, 3, 5] = np.nan
    t[4, 2, 6] = np.inf
    return [ball(c, "ones", tsdf=t, name="nonfinite/" + c) for c in BALL_CAMERAS]


def finite_cases():
    """every case the brute-force march and the restatement must agree on bit for bit"""
    return ball_cases() + slab_cases() + needle_cases() + crop_cases() + colour_cases()


def all_cases():
    return finite_cases() + nonfinite_cases()


# ---- the references of a case, computed once and shared by the host and the GPU tests; callers leave them unchanged
_REFERENCES = {}


class Reference:
    """depth, hit, s_hit and index of the brute-force march; restated depth, normals and hit count"""

    def __init__(self, case):
        import raycast_bruteforce as BF
        self.depth, self.hit, self.s_hit, self.index = BF.march(*case.args())
        with np.errstate(invalid="ignore", divide="ignore"):  # the non-finite scene's values
            self.restated_depth, self.normals, self.restated_hits = RC.raycast(
                case.tsdf, case.weight, case.K, case.twist, case.offset, case.voxel_size, case.image_shape,
                normals=True)
        self.hits = int(self.hit.sum())
        self.zero_normal = self.hit & ~self.normals.any(axis=2)


def reference(case):
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = Reference(case)
    return _REFERENCES[case.name]


def hole_crossings(case):
    """the number of rays with a valid, then an invalid, then a valid sample, all before their hit or their end"""
    import raycast_bruteforce as BF
    _, valid, _ = BF.trace(*case.args())
    before = np.arange(valid.shape[0])[:, None, None] <= reference(case).index[None]
    seen_valid = np.maximum.accumulate(valid & before, axis=0)
    seen_gap = np.maximum.accumulate(seen_valid & ~valid & before, axis=0)
    return int((seen_gap & valid & before).any(axis=0).sum())


def steps_needed(case):
    """the largest number of steps past its first that a lane of the kernel needs: the index of a ray's hit or last
    valid sample minus max(m_in - 2, 1), m_in its first sample inside the box.  The kernel starts at
    max(floor(lo / step) - 1, 1) and lo is no later than the first sample inside, so it starts no earlier"""
    import raycast_bruteforce as BF
    inside, _, _ = BF.trace(*case.args())
    index = reference(case).index
    first = np.where(inside.any(axis=0), inside.argmax(axis=0), 0)
    return int(np.where(index > 0, index - np.maximum(first - 2, 1), 0).max())


def colour_reference(case):
    """(image (H, W, 4) float32, valid (H, W) bool): photometric_restatement's colour step at the brute-force march's
    unrounded hit points, four NaNs where a pixel has no hit or no valid colour sample"""
    import photometric_restatement as P
    import raycast_bruteforce as BF
    ref = reference(case)
    a, b, _ = BF.ray(case.K, case.twist, case.offset, case.voxel_size, case.image_shape)
    rows, cols = np.nonzero(ref.hit)
    s = ref.s_hit[rows, cols]
    g = [a[j][rows, cols] + s * b[j][rows, cols] for j in range(3)]
    nz, ny, nx = case.tsdf.shape
    ok, rgb = P.sample_colour(case.colour, (nx, ny, nz), g)
    y = ((0.299 * rgb[0] + 0.587 * rgb[1]) + 0.114 * rgb[2]) / 255.0
    image = np.full(tuple(case.image_shape) + (4,), np.nan, np.float32)
    for ch, value in enumerate(rgb + [y]):
        image[rows[ok], cols[ok], ch] = value[ok].astype(np.float32)
    valid = np.zeros(case.image_shape, bool)
    valid[rows[ok], cols[ok]] = True
    return image, valid
