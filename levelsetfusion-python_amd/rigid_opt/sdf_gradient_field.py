"""calculate_gradient_wrt_twist (reference rigid_opt/sdf_gradient_field.py:13-38) as one HIP launch
(csrc/lsf_rigid.hip, mode GRADIENT; the kernel is the optimizer's).  The reference's quirks are kept:

* the "inverse" transform is twist_vector_to_matrix2d(-twist), which is not the inverse of twist_vector_to_matrix2d(twist);
* np.gradient: central differences inside, one-sided at the edges;
* the first term is [d/dx, d/dy] = [grad[1], grad[0]];
* the voxel point ((x + offset_x) * voxel_size, (y + offset_z) * voxel_size) is rounded to float32 before the float64
  product with the matrix;
* the float64 product is stored as float32 and then divided by voxel_size in float32."""
from .. import device_rigid


def calculate_gradient_wrt_twist(live_field, twist, array_offset, voxel_size=0.004, as_tensor=False):
    """(H, W, 3) float32 gradient of live_field (H, W) with respect to twist (t_x, t_z, theta); array_offset (3,) or
    (3, 1), fractional allowed.  as_tensor=True keeps it on the GPU."""
    g = device_rigid.gradient_wrt_twist(live_field, twist, array_offset, voxel_size)
    return g if as_tensor else g.cpu().numpy()


def calculate_gradient_wrt_twist_3d(live_field, twist, array_offset, voxel_size=0.004, as_tensor=False):
    """(Z, Y, X, 6) float32 gradient of the live volume (Z, Y, X) with respect to the 6-DoF twist (t_x, t_y, t_z, r_x,
    r_y, r_z): [grad ; p x grad] / voxel_size with p = twist_vector_to_matrix3d(-twist) . (point, 1), the 3-D form of
    calculate_gradient_wrt_twist.  One launch of csrc/lsf_rigid3d.hip, mode GRADIENT.
    as_tensor=True keeps it on the GPU."""
    g = device_rigid.gradient_wrt_twist_3d(live_field, twist, array_offset, voxel_size)
    return g if as_tensor else g.cpu().numpy()
