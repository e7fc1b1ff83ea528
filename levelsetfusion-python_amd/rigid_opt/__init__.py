"""SDF-2-SDF rigid 2-D tracking (reference rigid_opt/): Sdf2SdfOptimizer2d, its datasets and
calculate_gradient_wrt_twist.  The optimizer's whole loop runs on the GPU (csrc/lsf_rigid.hip)."""
