"""An RGB-D sensor in front of the fusion pipeline ("RGB-D sensor"; tests/rgbd_restatement.py
restates the kernels): a depth camera and, optionally, a colour camera with lenses of their own, a few centimetres apart
and of different resolutions.  RgbdSensor.register takes a raw frame pair and returns the depth registered into the
RECTIFIED colour camera, as an aligned stream of a sensor SDK is made, and the rectified colour image: both images of one
ideal pinhole camera, `sensor.camera`, which is what every tracker and fusion rule of this package assumes.  A pixel
without an answer -- disoccluded, outside the depth camera's view, or without a source in the rectified colour -- has depth
0, "no measurement" to every kernel that reads depth.  Without a colour camera the sensor rectifies the depth camera's own
lens.  The card's side is device_rgbd (csrc/lsf_rgbd.hip)."""
import numpy as np
import torch

from .. import device_rgbd
from ..device_core import require_gpu
from ..rigid_opt.frame_tracker import device_colour_image
from ..tsdf.generation import DepthCamera, device_depth

__all__ = ["RgbdSensor"]

EXTRINSICS = ("colour_to_depth", "depth_to_colour")


def _matrix_of(camera, name):
    try:
        K = camera.intrinsics.intrinsic_matrix
    except AttributeError:
        raise ValueError("%s must carry .intrinsics.intrinsic_matrix, got %r" % (name, camera)) from None
    device_rgbd.intrinsics(K, name + "'s intrinsic_matrix")
    return np.array(K, copy=True)


def _coefficients_of(camera):
    return device_rgbd.coefficients(getattr(camera.intrinsics, "distortion_coeffs", None))


def _camera_transform(camera):
    """the 4 x 4 of a camera's own extrinsics.rotation / .translation ("from camera 0 to camera 1"), None without them"""
    e = getattr(camera, "extrinsics", None)
    if e is None or getattr(e, "rotation", None) is None or getattr(e, "translation", None) is None:
        return None
    R, t = np.asarray(e.rotation, dtype=np.float64), np.asarray(e.translation, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or t.size != 3:
        raise ValueError("a camera's extrinsics are a 3 x 3 rotation and a translation of 3, got %s and %s"
                         % (R.shape, t.shape))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


class _Intrinsics:
    """what from_infinitam_format's cameras carry"""

    def __init__(self, resolution, intrinsic_matrix):
        self.resolution = resolution
        self.intrinsic_matrix = intrinsic_matrix
        self.distortion_coeffs = np.zeros((8, 1), np.float64)


class _Camera:
    def __init__(self, resolution, intrinsic_matrix, depth_unit_ratio=None):
        self.resolution = resolution
        self.intrinsics = _Intrinsics(resolution, intrinsic_matrix)
        if depth_unit_ratio is not None:
            self.depth_unit_ratio = depth_unit_ratio


class RgbdSensor:
    """depth_camera, colour_camera: any object with .intrinsics.intrinsic_matrix (3 x 3) and, optionally,
    .intrinsics.distortion_coeffs -- 0, 4, 5 or 8 OpenCV coefficients (k1, k2, p1, p2, k3, k4, k5, k6) in any shape; the
    depth camera also carries .depth_unit_ratio.  depth_to_colour: 4 x 4, q = R p + t from depth-camera to colour-camera
    coordinates; None takes the colour camera's extrinsics.rotation / .translation when it has them, else the identity.
    output_intrinsics: the matrix of the ideal output camera, the colour camera's by default (the depth camera's without
    a colour camera).  output_shape: (height, width) of the output; by default the colour image's extents at the first
    register (the depth image's without a colour camera).  max_footprint: the most output pixels per axis one depth
    pixel may cover (1 .. 16).  ray_tolerance_px: the ray tables are checked once per image size -- distorting the
    centre rays again must land within this many pixels of the pixel, else ValueError: a lens the fixed-point
    undistortion diverges on does not pass silently.  `camera` is the package's DepthCamera of the registered stream:
    the output matrix and depth_unit_ratio 1.0."""

    def __init__(self, depth_camera, colour_camera=None, depth_to_colour=None, output_intrinsics=None,
                 max_footprint=device_rgbd.DEFAULT_FOOTPRINT, ray_tolerance_px=1e-3, output_shape=None):
        self.depth_camera, self.colour_camera = depth_camera, colour_camera
        self.depth_matrix = _matrix_of(depth_camera, "depth_camera")
        self.depth_coefficients = _coefficients_of(depth_camera)
        try:
            self.depth_unit_ratio = float(depth_camera.depth_unit_ratio)
        except AttributeError:
            raise ValueError("depth_camera must carry .depth_unit_ratio") from None
        device_rgbd.params(depth_unit_ratio=self.depth_unit_ratio)
        if colour_camera is None:
            if depth_to_colour is not None:
                raise ValueError("depth_to_colour needs a colour_camera")
            self.colour_matrix, self.colour_coefficients = None, None
            self.depth_to_colour = np.eye(4)
            default_output = self.depth_matrix
        else:
            self.colour_matrix = _matrix_of(colour_camera, "colour_camera")
            self.colour_coefficients = _coefficients_of(colour_camera)
            own = _camera_transform(colour_camera) if depth_to_colour is None else None
            self.depth_to_colour = device_rgbd.transform_of(depth_to_colour) if depth_to_colour is not None else \
                (np.eye(4) if own is None else device_rgbd.transform_of(own, "the colour camera's extrinsics"))
            default_output = self.colour_matrix
        self.output_matrix = np.array(default_output if output_intrinsics is None else output_intrinsics, copy=True)
        device_rgbd.intrinsics(self.output_matrix, "output_intrinsics")
        self.max_footprint = device_rgbd.footprint_of(max_footprint)
        self.ray_tolerance_px = float(ray_tolerance_px)
        if not self.ray_tolerance_px > 0:
            raise ValueError("ray_tolerance_px must be > 0, got %r" % (ray_tolerance_px,))
        self.output_shape = None if output_shape is None else tuple(int(v) for v in output_shape)
        if self.output_shape is not None and (len(self.output_shape) != 2 or min(self.output_shape) < 1):
            raise ValueError("output_shape is (height, width) >= 1, got %r" % (output_shape,))
        self.camera = DepthCamera(intrinsics=DepthCamera.Intrinsics(intrinsic_matrix=self.output_matrix),
                                  depth_unit_ratio=1.0)
        # the colour image passes as it is: its lens is ideal and the output camera is the colour camera, bit for bit
        self.colour_passes = colour_camera is not None and not np.any(self.colour_coefficients != 0) and \
            self.output_matrix.dtype == self.colour_matrix.dtype and \
            self.output_matrix.tobytes() == self.colour_matrix.tobytes()
        self.depth_shape = self.colour_shape = None  # fixed by the first frame
        self.ray_residual_px = None  # of the last table check
        self._tables = self._zbuffer = None
        self.last_colour_valid = None

    # ---- host ---------------------------------------------------------------------------------------------------------

    def admit(self, depth_shape, colour_shape=None):
        """the host check of a frame's extents: the first call fixes them (and the output's), every later frame must
        have the same.  depth_shape: (H, W); colour_shape: (Hc, Wc) or (Hc, Wc, 3), None without a colour image"""
        depth_shape = tuple(int(v) for v in depth_shape)
        if len(depth_shape) != 2 or min(depth_shape) < 1:
            raise ValueError("the depth image must be 2-D with extents >= 1, got shape %s" % (depth_shape,))
        if colour_shape is not None:
            if self.colour_camera is None:
                raise ValueError("a colour image needs a sensor made with a colour_camera")
            colour_shape = tuple(int(v) for v in colour_shape)
            if len(colour_shape) == 3 and colour_shape[2] == 3:
                colour_shape = colour_shape[:2]
            if len(colour_shape) != 2 or min(colour_shape) < 1:
                raise ValueError("the colour image must be (H, W, 3) with extents >= 1, got shape %s" % (colour_shape,))
        if self.depth_shape is not None and depth_shape != self.depth_shape:
            raise ValueError("the depth image has extents %s, the sensor's first frame had %s"
                             % (depth_shape, self.depth_shape))
        if colour_shape is not None and self.colour_shape is not None and colour_shape != self.colour_shape:
            raise ValueError("the colour image has extents %s, the sensor's first colour frame had %s"
                             % (colour_shape, self.colour_shape))
        if self.output_shape is None:
            if self.colour_camera is None:
                self.output_shape = depth_shape
            elif colour_shape is not None:
                self.output_shape = colour_shape
            else:
                raise ValueError("a sensor with a colour_camera takes the output's extents from the first colour image; "
                                 "without one, give output_shape=(height, width)")
        self.depth_shape = depth_shape
        if colour_shape is not None:
            self.colour_shape = colour_shape

    @staticmethod
    def from_infinitam_format(path_or_handle, extrinsic="colour_to_depth", **settings):
        """the sensor of an InfiniTAM calib.txt: the colour size, `fx fy`, `cx cy`, a blank line; the same of the depth
        camera; three rows of a 3 x 4 transform, a blank line; the depth line, whose second token is the depth unit
        ratio (0 means 0.001).  InfiniTAM stores the colour-to-depth transform: depth_to_colour is its inverse, or,
        with extrinsic="depth_to_colour", the matrix as written.  The output has the file's colour size.  Host only."""
        if extrinsic not in EXTRINSICS:
            raise ValueError("extrinsic must be one of %s, got %r" % (EXTRINSICS, extrinsic))
        handle = open(path_or_handle, "r") if isinstance(path_or_handle, (str, bytes)) or \
            hasattr(path_or_handle, "__fspath__") else path_or_handle
        try:
            lines = [handle.readline() for _ in range(13)]
        finally:
            if handle is not path_or_handle:
                handle.close()
        numbers = lambda line: [float(v) for v in line.split()]

        def camera(block, ratio=None):
            try:
                (w, h), (fx, fy), (cx, cy) = (numbers(line) for line in block)
            except ValueError:
                raise ValueError("a camera of an InfiniTAM calibration is three lines of two numbers: the size, "
                                 "`fx fy`, `cx cy`; got %r" % (block,)) from None
            K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
            return _Camera((int(h), int(w)), K, ratio)

        rows = [numbers(line) for line in lines[8:11]]
        if any(len(r) != 4 for r in rows):
            raise ValueError("the transform of an InfiniTAM calibration is three rows of four numbers, got %r"
                             % (lines[8:11],))
        tokens = lines[12].strip().split(" ")
        if len(tokens) < 2:
            raise ValueError("the depth line of an InfiniTAM calibration holds the ratio as its second token, got %r"
                             % lines[12])
        ratio = float(tokens[1])
        if ratio == 0.0:
            ratio = 0.001
        written = np.vstack([np.array(rows, dtype=np.float64), [0.0, 0.0, 0.0, 1.0]])
        device_rgbd.transform_of(written, "the calibration's transform")
        colour, depth = camera(lines[0:3]), camera(lines[4:7], ratio)
        settings.setdefault("output_shape", colour.resolution)
        return RgbdSensor(depth, colour, written if extrinsic == "depth_to_colour" else np.linalg.inv(written),
                          **settings)

    # ---- the card -----------------------------------------------------------------------------------------------------

    def _ray_tables(self):
        """the depth camera's tables at the admitted extents, built and checked at the first use"""
        if self._tables is None:
            K, k, shape = self.depth_matrix, self.depth_coefficients, self.depth_shape
            corner, centre = device_rgbd.ray_table(shape, K, k)
            fx, fy, cx, cy = device_rgbd.intrinsics(K)
            k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in k)
            x, y = centre[..., 0], centre[..., 1]
            r2 = x * x + y * y
            s = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            xd = x * s + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
            yd = y * s + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
            u = torch.arange(shape[1], dtype=torch.float64, device=centre.device)[None, :]
            v = torch.arange(shape[0], dtype=torch.float64, device=centre.device)[:, None]
            miss = torch.maximum((fx * xd + cx - u).abs(), (fy * yd + cy - v).abs())
            miss = torch.where(torch.isfinite(miss), miss, torch.full_like(miss, float("inf")))
            self.ray_residual_px = float(miss.max().item())  # the one wait, once per image size
            if not self.ray_residual_px <= self.ray_tolerance_px:
                raise ValueError("the depth camera's undistorted rays, distorted again, miss their pixels by up to %g px "
                                 "(ray_tolerance_px = %g): the fixed-point undistortion does not converge on this lens"
                                 % (self.ray_residual_px, self.ray_tolerance_px))
            self._tables = (corner, centre)
        return self._tables

    def register_device(self, depth_image, colour_image=None):
        """register() with the record left on the card: (depth_m, colour, record int64 (8,) device tensor); nothing
        waits (but the first call's check of the ray tables)"""
        colour_shape = None if colour_image is None else tuple(colour_image.shape)
        self.admit(tuple(np.shape(depth_image)) if not isinstance(depth_image, torch.Tensor)
                   else tuple(depth_image.shape), colour_shape)
        require_gpu()
        depth, _ = device_depth(depth_image)
        corner, centre = self._ray_tables()
        colour, valid = None, None
        if colour_image is not None:
            colour = device_colour_image(colour_image)
            if colour.dim() != 3 or colour.shape[2] != 3 or colour.dtype != torch.uint8:
                raise ValueError("colour_image must be uint8 (H, W, 3), got %s %s" % (colour.dtype, tuple(colour.shape)))
            if not (self.colour_passes and tuple(colour.shape[:2]) == self.output_shape):
                colour, valid = device_rgbd.rectify_colour(colour.contiguous(), self.colour_matrix,
                                                           self.colour_coefficients, self.output_matrix,
                                                           self.output_shape)
        self.last_colour_valid = valid
        if self._zbuffer is None or self._zbuffer.device != depth.device:
            self._zbuffer = torch.empty(self.output_shape, dtype=torch.int32, device=depth.device)
        depth_m, record = device_rgbd.register_depth(depth, corner, centre, self.depth_to_colour, self.output_matrix,
                                                     self.output_shape, self.depth_unit_ratio, self.max_footprint,
                                                     valid, self._zbuffer)
        return depth_m, colour, record

    def register(self, depth_image, colour_image=None, record=False):
        """(depth_m, colour) of a raw frame pair: depth_m the float32 device image in metres of the depth registered
        into the output camera, colour the rectified uint8 (Ho, Wo, 3) device image, None without a colour_image.  When
        the colour lens is ideal and the output camera is the colour camera bit for bit the colour image is returned as
        it is: no launch, no colour_valid.  record=True adds the dict of the eight counts (device_rgbd.RECORD_FIELDS)
        as a third value, at the cost of one host wait"""
        depth_m, colour, rec = self.register_device(depth_image, colour_image)
        if not record:
            return depth_m, colour
        return depth_m, colour, device_rgbd.unpack_record(rec.cpu().numpy())
