"""Depth-image reading without cv2 (what rigid_opt/sdf_generation.py of the reference takes from cv2.imread(path, -1)
and cv2.cvtColor(..., COLOR_BGR2GRAY)).

* 16-bit (and 8-bit) PNG and other formats PIL knows: through PIL.
* OpenEXR: read_exr() below, numpy + zlib.  Single-part scanline files with NONE, ZIPS or ZIP compression and HALF or
  FLOAT channels; anything else (tiled, deep, multi-part, other compressions, UINT channels) is refused with a
  ValueError that names what was found.

read_depth_image() returns what the reference's image-based dataset builds: the image cast to uint16 (a C cast:
truncation toward zero), reduced to one channel, and 0 mapped to 65535.  "Gray" of an image whose B, G and R channels
are equal is that channel; an image whose colour channels differ is refused instead of guessing cv2's weights."""
import struct
import zlib

import numpy as np

EXR_MAGIC = 20000630
_COMPRESSIONS = {0: "NONE", 1: "RLE", 2: "ZIPS", 3: "ZIP", 4: "PIZ", 5: "PXR24", 6: "B44", 7: "B44A", 8: "DWAA",
                 9: "DWAB"}
_LINES_PER_CHUNK = {0: 1, 2: 1, 3: 16}
_PIXEL_TYPES = {1: ("HALF", np.dtype("<f2")), 2: ("FLOAT", np.dtype("<f4"))}


def _read_header(data, pos):
    attributes = {}
    while True:
        end = data.index(b"\0", pos)
        name = data[pos:end].decode("latin-1")
        pos = end + 1
        if not name:
            return attributes, pos
        end = data.index(b"\0", pos)
        kind = data[pos:end].decode("latin-1")
        pos = end + 1
        (size,) = struct.unpack_from("<i", data, pos)
        pos += 4
        attributes[name] = (kind, data[pos:pos + size])
        pos += size


def _channels(raw):
    out, pos = [], 0
    while raw[pos:pos + 1] != b"\0":
        end = raw.index(b"\0", pos)
        name = raw[pos:end].decode("latin-1")
        pos = end + 1
        pixel_type, _linear, x_sampling, y_sampling = struct.unpack_from("<iB3xii", raw, pos)
        pos += 16
        out.append((name, pixel_type, x_sampling, y_sampling))
    return out


def _unzip(chunk, raw_size):
    """zlib, then OpenEXR's byte predictor (t[i] += t[i-1] - 128) and the de-interleave of the two half buffers"""
    t = np.frombuffer(zlib.decompress(chunk), dtype=np.uint8)
    if t.size != raw_size:
        raise ValueError("EXR: a ZIP chunk inflates to %d bytes, expected %d" % (t.size, raw_size))
    d = t.astype(np.int64)
    d[1:] -= 128
    t = (np.cumsum(d) & 0xFF).astype(np.uint8)
    out = np.empty_like(t)
    half = (raw_size + 1) // 2
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def read_exr(path):
    """{channel name: float32 array [height][width]} of a scanline OpenEXR file"""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 8 or struct.unpack_from("<i", data, 0)[0] != EXR_MAGIC:
        raise ValueError("%s: not an OpenEXR file" % path)
    (flags,) = struct.unpack_from("<I", data, 4)
    if flags & 0xFF != 2:
        raise ValueError("%s: OpenEXR version %d is not supported" % (path, flags & 0xFF))
    if flags & 0x200:
        raise ValueError("%s: tiled OpenEXR files are not supported (scanline only)" % path)
    if flags & 0x800:
        raise ValueError("%s: deep OpenEXR files are not supported" % path)
    if flags & 0x1000:
        raise ValueError("%s: multi-part OpenEXR files are not supported" % path)
    attributes, pos = _read_header(data, 8)
    compression = attributes["compression"][1][0]
    if compression not in _LINES_PER_CHUNK:
        raise ValueError("%s: OpenEXR compression %s is not supported (NONE, ZIPS, ZIP only)"
                         % (path, _COMPRESSIONS.get(compression, compression)))
    x_min, y_min, x_max, y_max = struct.unpack("<iiii", attributes["dataWindow"][1])
    width, height = x_max - x_min + 1, y_max - y_min + 1
    channels = _channels(attributes["channels"][1])
    for name, pixel_type, xs, ys in channels:
        if pixel_type not in _PIXEL_TYPES:
            raise ValueError("%s: channel %s has pixel type %d; only HALF and FLOAT are supported"
                             % (path, name, pixel_type))
        if xs != 1 or ys != 1:
            raise ValueError("%s: channel %s is subsampled, which is not supported" % (path, name))
    lines = _LINES_PER_CHUNK[compression]
    n_chunks = (height + lines - 1) // lines
    offsets = struct.unpack_from("<%dQ" % n_chunks, data, pos)
    row_bytes = sum(_PIXEL_TYPES[c[1]][1].itemsize for c in channels) * width
    planes = {c[0]: np.empty((height, width), dtype=np.float32) for c in channels}
    for offset in offsets:
        y, size = struct.unpack_from("<ii", data, offset)
        chunk = data[offset + 8:offset + 8 + size]
        rows = min(lines, y_max + 1 - y)
        raw_size = rows * row_bytes
        raw = chunk if (compression == 0 or size >= raw_size) else _unzip(chunk, raw_size)
        if len(raw) != raw_size:
            raise ValueError("%s: truncated chunk at line %d" % (path, y))
        p = 0
        for r in range(rows):
            for name, pixel_type, _, _ in channels:
                dt = _PIXEL_TYPES[pixel_type][1]
                n = width * dt.itemsize
                planes[name][y - y_min + r] = np.frombuffer(raw, dtype=dt, count=width, offset=p)
                p += n
    return planes


def read_image(path):
    """the image as cv2.imread(path, -1) gives it: [height][width] for one channel, [height][width][C] with colour
    channels in B, G, R(, A) order otherwise; EXR as float32"""
    if str(path).lower().endswith(".exr"):
        planes = read_exr(path)
        if len(planes) == 1:
            return next(iter(planes.values()))
        order = [c for c in ("B", "G", "R", "A") if c in planes]
        if len(order) != len(planes):
            raise ValueError("%s: channels %s are not B, G, R(, A)" % (path, sorted(planes)))
        return np.stack([planes[c] for c in order], axis=-1)
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim == 3:  # PIL gives RGB(A); cv2 gives BGR(A)
        a = a[..., [2, 1, 0] + ([3] if a.shape[2] == 4 else [])]
    return a


def to_gray(image):
    """one channel of an image whose colour channels are equal (what COLOR_BGR2GRAY gives for it); a 2-D image as is"""
    if image.ndim == 2:
        return image
    if image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError("expected a [height][width] or [height][width][3|4] image, got shape %s" % (image.shape,))
    b, g, r = image[..., 0], image[..., 1], image[..., 2]
    if not (np.array_equal(b, g) and np.array_equal(b, r)):
        raise ValueError("colour image: its B, G and R channels differ, and cv2's gray weights are not restated here")
    return np.ascontiguousarray(b)


def read_depth_image(path):
    """uint16 depth as the reference's ImageBasedSingleFrameDataset builds it: astype(uint16), gray, 0 -> 65535"""
    image = read_image(path)
    with np.errstate(invalid="ignore"):
        depth = to_gray(image.astype(np.uint16))
    depth = depth.copy()
    depth[depth == 0] = np.iinfo(np.uint16).max
    return depth
