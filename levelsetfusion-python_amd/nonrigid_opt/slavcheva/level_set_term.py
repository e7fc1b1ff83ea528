"""Level-set term of the Slavcheva-style energy at one location (reference: nonrigid_opt/slavcheva/level_set_term.py).
The optimizers run the term inside their fused HIP kernels; this function runs it on its own (csrc/lsf_terms.hip,
lsf_term_gradient).  numpy in, numpy out; a ROCm tensor in, a gradient tensor on the device out.  (The reference's
whole-field level_set_term_gradient is an empty stub and has no counterpart here.)"""
from ... import _lib
from ...device_terms import term_at


def level_set_term_at_location(warped_live_field, x, y, epsilon=1e-5):
    """level_set_term.py:28-64: (1 - |g|) / (|g| + epsilon) * H g with g the central-difference gradient and H the Hessian,
    both times 10; neighbours outside the array read 1, and grad_xx / grad_yy use the +1 neighbour twice, as in the
    reference.  Returns (gradient, 0.5 (|g| - 1)^2).  One launch and one wait for the device per call."""
    return term_at(_lib.TERM_LEVEL_SET, x, y, warped_live_field, epsilon=epsilon)
