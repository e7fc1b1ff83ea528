"""Smoothing term of the Slavcheva-style energy (reference: nonrigid_opt/slavcheva/smoothing_term.py): the method
selector the optimizers take -- Tikhonov = -Laplacian of the previous update, Killing = approximately-Killing-vector-field
regulariser, both run inside the optimizers' HIP kernels (csrc/lsf_slavcheva.hip) -- and the term-level functions with
the reference's names, signatures and defaults, which run one term on its own (csrc/lsf_terms.hip, lsf_term_gradient).

numpy in, numpy out (gradients float32, (H, W, 2) or (D, H, W, 3)); ROCm tensors in, tensors on the device out.  The
whole-field functions are one launch and also take 3-D fields; the per-location functions are 2-D, as in the reference,
and so are copy_if_zero / ignore_if_zero."""
from enum import Enum

from ... import _lib
from ...device_terms import term_at, term_field


class SmoothingTermMethod(Enum):
    TIKHONOV = 0
    KILLING = 1


# ------------------------------------------------------------------------------------------- at one location (2-D)
def compute_local_smoothing_term_gradient_killing(warp_field, x, y, ignore_if_zero=False, copy_if_zero=True,
                                                  isomorphic_enforcement_factor=0.1):
    """smoothing_term.py:50-100, every quirk kept: w_yy uses the +1 neighbour twice and -2(1 + lambda) multiplies the xx
    term only; ignore_if_zero is accepted and ignored, as in the reference.  copy_if_zero: a neighbour outside the array
    or of norm 0 reads the centre value (otherwise only one outside the array does).  Returns (gradient, local energy).
    One launch and one wait for the device per call."""
    return term_at(_lib.TERM_KILLING, x, y, warp=warp_field, copy_if_zero=copy_if_zero,
                   isomorphic_enforcement_factor=isomorphic_enforcement_factor)


def compute_local_smoothing_term_gradient_tikhonov(warp_field, x, y, ignore_if_zero=False, copy_if_zero=True,
                                                   isomorphic_enforcement_factor=0.1):
    """smoothing_term.py:103-139: -(w[x+1] + w[y+1] - 4 w + w[x-1] + w[y-1]) and 0.5 (|w_x|^2 + |w_y|^2).
    ignore_if_zero: (0, 0) and energy 0 where ANY component of an existing 4-neighbour is 0 (the reference takes the norm
    of a boolean vector).  copy_if_zero as for Killing.  One launch and one wait for the device per call."""
    return term_at(_lib.TERM_TIKHONOV_LOCAL, x, y, warp=warp_field, copy_if_zero=copy_if_zero,
                   ignore_if_zero=ignore_if_zero)


smoothing_term_methods = {SmoothingTermMethod.KILLING: compute_local_smoothing_term_gradient_killing,
                          SmoothingTermMethod.TIKHONOV: compute_local_smoothing_term_gradient_tikhonov}


def compute_local_smoothing_term_gradient(warp_field, x, y, ignore_if_zero=False,
                                          copy_if_zero=True, method=SmoothingTermMethod.TIKHONOV,
                                          isomorphic_enforcement_factor=0.1):
    """smoothing_term.py:146-149.  One launch and one wait for the device per call."""
    return smoothing_term_methods[method](warp_field, x, y, ignore_if_zero, copy_if_zero, isomorphic_enforcement_factor)


# ------------------------------------------------------------------------------------------------- whole fields
def compute_smoothing_term_gradient_vectorized(warp_field):
    """smoothing_term.py:155-159: -scipy.ndimage.laplace of every component (edge replicated).  One launch."""
    return term_field(_lib.TERM_TIKHONOV, warp=warp_field)[0]


def compute_smoothing_term_energy(warp_field, warped_live_field=None, canonical_field=None, band_union_only=True):
    """smoothing_term.py:162-177: 0.5 * sum of the squared np.gradient of every component (over the narrow-band union),
    summed in float64.  One launch; waits for the device."""
    if band_union_only and (warped_live_field is None or canonical_field is None):
        raise ValueError(
            "To determine the narrow band union, warped_live_field and canonical_field should be defined."
            " Otherwise, please set the 'band_union_only argument' to 'False'")
    return term_field(_lib.TERM_TIKHONOV, warped_live_field if band_union_only else None,
                      canonical_field if band_union_only else None, warp=warp_field, band=band_union_only,
                      want_gradient=False, want_energy=True, energy_form=_lib.TERM_ENERGY_NP_GRADIENT)[1]


def compute_smoothing_term_gradient_direct(warp_field, warped_live_field, canonical_field, band_union_only=True):
    """smoothing_term.py:180-201: (gradient field, total energy) of the per-location Tikhonov term (copy_if_zero off)
    at every voxel; with band_union_only voxels outside the narrow-band union get gradient 0 and add no energy.
    One launch; waits for the device for the energy."""
    if band_union_only and (warped_live_field is None or canonical_field is None):
        raise ValueError("band_union_only needs warped_live_field and canonical_field")
    return term_field(_lib.TERM_TIKHONOV_LOCAL, warped_live_field if band_union_only else None,
                      canonical_field if band_union_only else None, warp=warp_field, band=band_union_only,
                      want_energy=True)
