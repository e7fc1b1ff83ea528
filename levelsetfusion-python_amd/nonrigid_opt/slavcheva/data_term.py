"""Data term of the Slavcheva-style energy (reference: nonrigid_opt/slavcheva/data_term.py): the method selector the
optimizers take, and the term-level functions with the reference's names, signatures and defaults.  The optimizers run
the term inside their fused HIP kernels (csrc/lsf_slavcheva.hip); the functions below run it on its own
(csrc/lsf_terms.hip, lsf_term_gradient).

numpy in, numpy out (gradients float32, (H, W, 2) or (D, H, W, 3)); ROCm tensors in, tensors on the device out.  The
whole-field functions are one launch and also take 3-D fields (pass live_gradient_z); the per-location functions are
2-D, as in the reference."""
from enum import Enum

from ... import _lib
from ...device_terms import term_at, term_field


class DataTermMethod(Enum):
    BASIC = 0
    BASIC_CPP = 1          # the reference's C++ twin of BASIC; identical arithmetic here
    THRESHOLDED_FDM = 2    # the threshold picks the finite-difference direction (data_term.py:190-227)


def _gradients(live_gradient_x, live_gradient_y, live_gradient_z):
    return (live_gradient_x, live_gradient_y) + ((live_gradient_z,) if live_gradient_z is not None else ())


# ------------------------------------------------------------------------------------------- at one location (2-D)
def compute_local_data_term_gradient_basic(warped_live_field, canonical_field, x, y, live_gradient_x, live_gradient_y):
    """data_term.py:169-187: ((live - canonical) * caller gradient at (x, y) * 10, 0.5 (live - canonical)^2).
    One launch and one wait for the device per call."""
    return term_at(_lib.TERM_DATA_BASIC, x, y, warped_live_field, canonical_field,
                   (live_gradient_x, live_gradient_y), scaling_factor=10.0)


def compute_local_data_term_gradient_thresholded_fdm(warped_live_field, canonical_field, x, y, live_gradient_x,
                                                     live_gradient_y):
    """data_term.py:190-227: a caller gradient component above 0.5 is replaced by the smaller one-sided difference (the
    backward one on a tie; neighbours outside the array read 1), and by 0 if that too is above 0.5.
    One launch and one wait for the device per call."""
    return term_at(_lib.TERM_DATA_THRESHOLDED_FDM, x, y, warped_live_field, canonical_field,
                   (live_gradient_x, live_gradient_y), scaling_factor=10.0)


def data_term_at_location(warped_live_field, canonical_field, x, y, live_gradient_x, live_gradient_y):
    """the reference's C++ twin of compute_local_data_term_gradient_basic (DataTermMethod.BASIC_CPP): the same result.
    One launch and one wait for the device per call."""
    return compute_local_data_term_gradient_basic(warped_live_field, canonical_field, x, y, live_gradient_x,
                                                  live_gradient_y)


data_term_methods = {DataTermMethod.BASIC: compute_local_data_term_gradient_basic,
                     DataTermMethod.THRESHOLDED_FDM: compute_local_data_term_gradient_thresholded_fdm,
                     DataTermMethod.BASIC_CPP: data_term_at_location}


def compute_local_data_term(warped_live_field, canonical_field, x, y, live_gradient_x, live_gradient_y,
                            method=DataTermMethod.BASIC):
    """data_term.py:235-237.  One launch and one wait for the device per call."""
    return data_term_methods[method](warped_live_field, canonical_field, x, y, live_gradient_x, live_gradient_y)


# ------------------------------------------------------------------------------------------------- whole fields
def compute_data_term_gradient_vectorized(warped_live_field, canonical_field, live_gradient_x, live_gradient_y,
                                          scaling_factor=10.0, live_gradient_z=None):
    """data_term.py:334-349: (live - canonical) * caller gradient * scaling_factor at every voxel.  One launch."""
    return term_field(_lib.TERM_DATA_BASIC, warped_live_field, canonical_field,
                      _gradients(live_gradient_x, live_gradient_y, live_gradient_z),
                      scaling_factor=scaling_factor)[0]


def compute_data_term_energy_contribution(warped_live_field, canonical_field, band_union_only=True):
    """data_term.py:352-358: sum of 0.5 (live - canonical)^2 (over the narrow-band union), summed in float64.
    One launch; waits for the device."""
    return term_field(_lib.TERM_DATA_BASIC, warped_live_field, canonical_field, band=band_union_only,
                      want_gradient=False, want_energy=True)[1]


def compute_data_term_gradient_direct(warped_live_field, canonical_field, live_gradient_x, live_gradient_y,
                                      band_union_only=True, live_gradient_z=None):
    """data_term.py:361-384: (gradient field, total energy) of the BASIC term; with band_union_only voxels outside the
    narrow-band union get gradient 0 and add no energy.  One launch; waits for the device for the energy."""
    return term_field(_lib.TERM_DATA_BASIC, warped_live_field, canonical_field,
                      _gradients(live_gradient_x, live_gradient_y, live_gradient_z), band=band_union_only,
                      want_energy=True, scaling_factor=10.0)
