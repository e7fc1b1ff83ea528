"""Twist vectors to homogeneous matrices (reference math_utils/transformation.py:11-34), host numpy.

The 3-D form needs Rodrigues' formula, which the reference takes from cv2.Rodrigues; it is restated here in numpy with
OpenCV's operation order -- theta = |r|, identity below DBL_EPSILON, otherwise u = r * (1 / theta) and
R = (cos(theta) I + (1 - cos(theta)) u u^T) + sin(theta) [u]_x in float64 -- and, as OpenCV does, rounded to the dtype of
a float32 input.  Both functions return float64 matrices, as the reference's do."""
import math

import numpy as np


def twist_vector_to_matrix2d(twist):
    """(tx, ty, theta) -> 3x3 float64 [[cos, -sin, tx], [sin, cos, ty], [0, 0, 1]]"""
    theta = float(np.asarray(twist[2]).reshape(-1)[0])
    twist_matrix = np.identity(3)
    twist_matrix[0, 0] = math.cos(theta)
    twist_matrix[0, 1] = -math.sin(theta)
    twist_matrix[1, 0] = math.sin(theta)
    twist_matrix[1, 1] = math.cos(theta)
    twist_matrix[0, 2] = np.asarray(twist[0]).reshape(-1)[0]
    twist_matrix[1, 2] = np.asarray(twist[1]).reshape(-1)[0]
    return twist_matrix


def rodrigues(rotation_vector):
    """3x3 rotation matrix of a rotation vector, in the vector's float dtype (float32 stays float32, anything else is
    float64), evaluated in float64 -- what cv2.Rodrigues returns for a 3-vector"""
    r = np.asarray(rotation_vector)
    dtype = np.float32 if r.dtype == np.float32 else np.float64
    r = r.astype(np.float64).reshape(-1)
    if r.size != 3:
        raise ValueError("rotation vector must have 3 entries, got %d" % r.size)
    theta = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if theta < np.finfo(np.float64).eps:
        return np.eye(3, dtype=dtype)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    itheta = 1.0 / theta
    u = r * itheta
    cross = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    rotation = (c * np.eye(3) + c1 * np.outer(u, u)) + s * cross
    return rotation.astype(dtype)


def twist_vector_to_matrix3d(twist):
    """(tx, ty, tz, rx, ry, rz), shape (6, 1) or (6,) -> 4x4 float64 [[R, t], [0, 1]]; R by rodrigues() of the rotation
    part (rounded to float32 when the twist is float32), t the translation part in the twist's dtype"""
    t = np.asarray(twist)
    if t.size != 6:
        raise ValueError("twist must have 6 entries, got %d" % t.size)
    if t.dtype != np.float32:
        t = t.astype(np.float64)
    t = t.reshape(6)
    matrix = np.zeros((4, 4))
    matrix[0:3, 0:3] = rodrigues(t[3:6])
    matrix[0:3, 3] = t[0:3]
    matrix[3, 3] = 1.0
    return matrix
