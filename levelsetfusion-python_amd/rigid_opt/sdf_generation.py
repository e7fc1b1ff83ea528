"""The rigid tracker's datasets (reference rigid_opt/sdf_generation.py): a canonical and a live 2-D TSDF row slice from
two depth images, the live one under a 6-vector twist.

Fields are generated on the GPU by the nearest-pixel generator on the reference's dtypes
(tsdf.generation.generate_tsdf_field_from_depth_image_typed): float64 extrinsic from twist_vector_to_matrix3d, fractional
offsets such as (-16, -16, 93.4375), uint16 or float depth.  Other filtering methods go through the package's
dispatcher.  ImageBasedSingleFrameDataset reads its frames without cv2 (image_io.read_depth_image): astype(uint16),
gray, 0 -> 65535, as the reference does."""
import numpy as np

from .. import image_io
from ..math_utils.transformation import twist_vector_to_matrix3d
from ..tsdf import generation as tsdf_gen
from ..tsdf.generation import FilteringMethod


def _generate(depth_image, camera, image_pixel_row, field_size, offset, narrow_band_width_voxels, method,
              camera_extrinsic_matrix=None, as_tensor=False):
    if method == FilteringMethod.NONE:
        return tsdf_gen.generate_tsdf_field_from_depth_image_typed(
            depth_image, camera, image_pixel_row, camera_extrinsic_matrix=camera_extrinsic_matrix,
            field_size=field_size, array_offset=offset, narrow_band_width_voxels=narrow_band_width_voxels,
            as_tensor=as_tensor)
    return tsdf_gen.generate_2d_tsdf_field_from_depth_image(
        depth_image, camera, image_pixel_row, camera_extrinsic_matrix=camera_extrinsic_matrix, field_size=field_size,
        array_offset=offset, narrow_band_width_voxels=narrow_band_width_voxels, interpolation_method=method,
        as_tensor=as_tensor)


class _SingleFrameDataset:
    """the shared half: generate_2d_canonical_field / generate_2d_live_field / generate_2d_sdf_fields on
    canonical_depth_image() and live_depth_image()"""

    def generate_2d_sdf_fields(self, narrow_band_width_voxels=20., method=FilteringMethod.NONE):
        canonical_field = self.generate_2d_canonical_field(narrow_band_width_voxels=narrow_band_width_voxels,
                                                           method=method)
        live_field = self.generate_2d_live_field(narrow_band_width_voxels=narrow_band_width_voxels, method=method)
        return live_field, canonical_field

    def generate_2d_canonical_field(self, narrow_band_width_voxels=20., method=FilteringMethod.NONE, as_tensor=False):
        return _generate(self.canonical_depth_image(), self.depth_camera, self.image_pixel_row, self.field_size,
                         self.offset, narrow_band_width_voxels, method, as_tensor=as_tensor)

    def generate_2d_live_field(self, method=FilteringMethod.NONE, narrow_band_width_voxels=20.,
                               twist=np.zeros((6, 1)), as_tensor=False):
        return _generate(self.live_depth_image(), self.depth_camera, self.image_pixel_row, self.field_size,
                         self.offset, narrow_band_width_voxels, method, twist_vector_to_matrix3d(twist),
                         as_tensor=as_tensor)


class ImageBasedSingleFrameDataset(_SingleFrameDataset):
    def __init__(self, first_frame_path, second_frame_path, image_pixel_row, field_size, offset, camera):
        self.first_frame_path = first_frame_path
        self.second_frame_path = second_frame_path
        self.image_pixel_row = image_pixel_row
        self.field_size = field_size
        self.offset = offset
        self.depth_camera = camera

    def canonical_depth_image(self):
        return image_io.read_depth_image(self.first_frame_path)

    def live_depth_image(self):
        return image_io.read_depth_image(self.second_frame_path)


class ArrayBasedSingleFrameDataset(_SingleFrameDataset):
    def __init__(self, depth_image0, depth_image1, image_pixel_row, field_size, offset, camera):
        self.depth_image0 = depth_image0
        self.depth_image1 = depth_image1
        self.image_pixel_row = image_pixel_row
        self.field_size = field_size
        self.offset = offset
        self.depth_camera = camera

    def canonical_depth_image(self):
        return self.depth_image0

    def live_depth_image(self):
        return self.depth_image1
