"""Device-resident optimizer engines (dimension-generic, slab-aware).  The drop-in classes under nonrigid_opt/ are thin
shells around these.

All state lives in torch ROCm tensors; every per-voxel operation is a hand-written HIP kernel reached through the C ABI
(device.py -> liblsf_hip.so).  The host only enqueues launches -- or hands a whole call to the library -- and reads back
the tiny iteration records to learn whether the device-side convergence gate has closed.

This module is the import point; the code lives in
    engine_common.py     input conversion, pyramid level rule, graph-capture lock, the one shape of engine._fast
    engine_options.py    the knobs that are not part of the reference's signatures, and the last call's report
    engine_hier.py       HierarchicalEngine: a level and its filter plan, the eager / HIP-graph / blocked 2-D / z-slab
                         drivers, the level outcome they all return and the results and reports made of it
    engine_hier_pyramid.py  ... its canonical / live pyramids (whole volumes and z-slabs)
    engine_slavcheva.py  SlavchevaEngine: construction and declared state, the route of a call (_route, last_call.route) and
                         the launch-by-launch sub-decisions (_launch_plan), that call as stages over one iteration object
                         (the fused-state one lives here), hooks, gradient_field
    engine_run.py        ... the setup and epilogue the library-enqueued calls share (_RunCall) and the whole-volume call
                         (fixed-count, threshold-terminated, SobolevFusion)
    engine_slab.py       ... on z- / y-slabs: launch plan, exchange groups, compact faces, the library-enqueued slab call,
                         the wider re-run
    engine_sobolev.py    ... the SobolevFusion iteration objects (float4 lists / boxes, planar fields)
    engine_outcome.py    what a call leaves behind: final fields on demand, the per-iteration log, the gradient source
                         (recompute_gradient, kept as an engine_common._Lazy), what the iterations on the float4 states share
"""
from .engine_common import as_device_field, pyramid_level_count  # noqa: F401
from .engine_hier import HierarchicalEngine, LevelResult  # noqa: F401
from .engine_outcome import SlavchevaOutcome  # noqa: F401
from .engine_slavcheva import SlavchevaEngine  # noqa: F401
