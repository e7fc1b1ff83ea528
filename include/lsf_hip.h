/*
 * lsf_hip.h -- C ABI of liblsf_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the per-voxel
 * warp-field gradient-descent path of KillingFusion / SobolevFusion-style non-rigid TSDF alignment.
 *
 * This is the drop-in boundary under the Python classes SlavchevaOptimizer2d / HierarchicalOptimizer2d/3d.
 * The reference (Algomorph/LevelSetFusion-Python) crosses its only language boundary through a boost-python
 * module `level_set_fusion_optimization` (un-vendored C++); the entry points below are what a binding for
 * THIS path binds instead.  Each one names the reference interface it replaces (path:line under the
 * reference checkout).
 *
 * Rules of the ABI
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on success or a
 *     hipError_t value; nothing throws.  LSF_ERR_* (negative) flag argument errors detected on the host.
 *   - The library owns no FIELD memory: every field, state, list, record and scratch buffer is the caller's.  What it
 *     does own: per slab communicator (lsf_slab_comm_create ... _destroy) a HIP stream, a few events and two small
 *     face-count buffers (one hipMalloc, one hipHostMalloc); per host thread and device one timing-less event
 *     (lsf_state_run_begin).  Its only process-wide state is read-only after first use: the table of RCCL entry points
 *     the z-slab runtime binds once (under a mutex) and per-device cached device attributes.  All field pointers are
 *     DEVICE pointers supplied by the caller (e.g. torch.Tensor.data_ptr()), all launches are asynchronous on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream); the functions that also WAIT say so
 *     (lsf_state_run_begin / _finish, lsf_slab_face_counts_end).  Re-entrant across streams, devices and host threads.
 *   - Layouts (MI355X-first):
 *       scalar fields      float32 [z][y][x]            (nz = 1 for 2-D)
 *       vector fields      float32 PLANAR [c][z][y][x]  c = 0:x(u) 1:y(v) 2:z(w); `dims` planes
 *       packed live field  float4  [z][y][x] = (live, d/dx live, d/dy live, d/dz live)   (gather operand)
 *       interleaved        float32 [z][y][x][c]         only at the API edge (lsf_interleave/deinterleave)
 *   - Slab support: a launch processes slices z in [z_begin, z_end) of an array that holds nz slices
 *     (owned slab + halo).  z_global_offset is added to z when a voxel index is reported (arg-max).
 *   - Arithmetic: float32, multiply and add rounded separately (-ffp-contract=off), in the operation order
 *     of oracle/lsf_oracle.py, so results are bit-identical to the oracle except for sum reductions.
 */
#ifndef LSF_HIP_H
#define LSF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSF_ABI_VERSION 4
#define LSF_MAX_KERNEL_TAPS 31

#define LSF_ERR_BAD_ARGUMENT (-1)
#define LSF_ERR_BAD_DIMS (-2)
#define LSF_ERR_KERNEL_TOO_LONG (-3)
#define LSF_ERR_RCCL_UNAVAILABLE (-4) /* librccl.so could not be bound at run time */
#define LSF_ERR_RCCL_FAILED (-5)      /* an RCCL call returned an error (its text goes to stderr) */
#define LSF_ERR_NOT_RESIDENT (-6)     /* lsf_hip_chain.h: the chain kernel's workgroups cannot all be resident on this device */

/* extents of one field as stored on this device */
typedef struct lsf_grid {
    int32_t dims;            /* 2 or 3 */
    int32_t nz, ny, nx;      /* allocated extents, nz = 1 when dims == 2 */
    int32_t z_begin, z_end;  /* slices processed by the launch, 0 <= z_begin <= z_end <= nz */
    int32_t z_global_offset; /* global z of local slice 0 (for reported voxel indices) */
    int32_t y_global_offset; /* global y of local row 0: slabs cut along y; 0 otherwise */
    /* lsf_slavcheva_state_iteration only: energies are accumulated for slices in [energy_z_begin, energy_z_end) --
     * a z-slab launch that recomputes halo slices must not count them twice.
     * energy_z_end <= energy_z_begin (e.g. both 0): every slice of the launch counts. */
    int32_t energy_z_begin, energy_z_end;
    /* Slabs cut along y (lsf_slavcheva_state_iteration on band lists and lsf_state_finalize_listed honour these; every
     * other entry point requires y_global_offset == 0 and ny_global in {0, ny}): the local array holds rows
     * [y_global_offset, y_global_offset + ny) of a volume with ny_global rows (0 = ny: not cut along y).  Reported voxel
     * indices are ((z + z_global_offset) * ny_global + y + y_global_offset) * nx + x, gather positions are formed from the
     * GLOBAL row (float32(y + y_global_offset) + displacement, as with z), and energies count rows in
     * [energy_y_begin, energy_y_end) only (energy_y_end <= energy_y_begin: every row). */
    int32_t ny_global;
    int32_t energy_y_begin, energy_y_end;
} lsf_grid;

/* per-iteration reduction record written by the iteration kernels (one record per iteration).
 * max_packed = (float bits of the maximum vector length << 32) | ~(linear voxel index): the largest value
 * with the smallest index wins an unsigned 64-bit max, which reproduces numpy's first-arg-max tie break
 * (hierarchical_optimizer2d.py:223-225, slavcheva_optimizer2d.py:213-215).  0 = iteration not executed.
 *
 * A record is kept as LSF_RECORD_SLOTS partial records 4 KiB apart (different memory channels); a block accumulates into slot
 * (block id mod 8), i.e. the slot of its XCD.  The record's VALUE is the max over the slots' max_packed and the sum
 * over the slots' energies -- the gate below, and the host when it decodes records, combine them that way.  (Atomics
 * of ~2000 blocks on one address serialise at ~12 ns each: 0.10 -> 0.055 ms for the band-list kernel at 256^3.) */
#define LSF_RECORD_SLOTS 8
typedef struct lsf_record_slot {
    uint64_t max_packed;
    double data_energy;      /* Slavcheva: sum over band of 0.5*diff^2 ; hierarchical: sum diff^2 */
    double smoothing_energy; /* un-weighted */
    double level_set_energy; /* un-weighted */
    uint64_t pad[508];
} lsf_record_slot; /* 4096 bytes: the slots of a record land in different L2 / memory channels (256 bytes apart, the
                      eight atomics streams of a launch's ~1000 blocks shared one: 0.0368 -> 0.0353 ms at 256^3) */
typedef struct lsf_iteration_record {
    lsf_record_slot slot[LSF_RECORD_SLOTS];
} lsf_iteration_record; /* 32 KiB */

/* HOST-side reading of records that have been copied to the host (no device involved): the value of each of n records,
 * combined over its partial slots as above.  slots = n x n_slots x slot_words int64 words, the first four words of every
 * slot being max_packed and the three energies (slot_words >= 4: 512 for whole records, 4 when only the used words were
 * copied; n_slots = LSF_RECORD_SLOTS, or a multiple of it when the slots of several ranks' records stand side by side).
 * Out, n entries each (energies3: n x 3): the maximum as a float, the voxel index it was found at, the energy sums
 * (slots added in ascending order), executed = 1 where the record's maximum word is non-zero. */
int lsf_records_decode(const int64_t *slots, int32_t n, int32_t n_slots, int32_t slot_words, float *max_value,
                       int64_t *argmax, double *energies3, uint8_t *executed);

/* Device-side convergence gate.  The reference tests its stop condition on the host after every iteration
 * (hierarchical_optimizer2d.py:169-171, slavcheva_optimizer2d.py:360-362); here every kernel of iteration i
 * looks at the record of iteration i-1 and turns itself into a no-op when that iteration already met the
 * stop condition (or was itself a no-op), so the host may enqueue iterations in batches without a sync and
 * still get exactly the reference's iteration count.  prev_record == NULL: always run.
 *   mode LSF_GATE_HIERARCHICAL: run iff NOT (max < a)            (a = maximum_warp_update_threshold)
 *   mode LSF_GATE_SLAVCHEVA:    run iff  a < max  AND  max < b   (a, b = lower / upper warp thresholds) */
#define LSF_GATE_HIERARCHICAL 0
#define LSF_GATE_SLAVCHEVA 1
#define LSF_GATE_OPEN 2 /* never closes; only names the previous record (lsf_hier_params::previous_max) */
typedef struct lsf_gate {
    const lsf_iteration_record *prev_record; /* DEVICE pointer or NULL */
    int32_t mode;
    float a;
    float b;
} lsf_gate;

/* ---------------------------------------------------------------------------------------------------- */
int lsf_abi_version(void);
/* first 16 hex digits of the SHA-256 over the NORMALISED text of this header (comments stripped, white space collapsed:
 * _build.py::abi_hash) as it stood when the library was compiled -- every struct and prototype goes into it, so a
 * binding written against another revision of the header is refused at load time (levelsetfusion-python_amd/_lib.py
 * compares it with the hash of the header it was written against) whether or not someone remembered to bump
 * LSF_ABI_VERSION.  "unknown" when compiled by hand. */
const char *lsf_abi_hash(void);
/* name of the code object's target, e.g. "gfx950" */
const char *lsf_target_arch(void);
/* identity of the build: the first 16 hex digits of the SHA-256 over the library's sources (csrc/, include/), set by the
 * build script; "unknown" when compiled by hand.  bench.py reports the committed rocprofv3 HBM-traffic figures only for
 * the build they were measured on (profiles/traffic.json carries the id). */
const char *lsf_build_id(void);

/* ---- layout helpers (API edge only) ---------------------------------------------------------------- */
/* [z][y][x][c] -> [c][z][y][x] and back; n_voxels = nz*ny*nx, channels = dims */
int lsf_deinterleave(const float *interleaved, float *planar, int64_t n_voxels, int32_t channels, void *stream);
int lsf_interleave(const float *planar, float *interleaved, int64_t n_voxels, int32_t channels, void *stream);

/* ---- z-slab halo staging (new design; the reference has no distributed code) -----------------
 * Copies `halo` consecutive slices starting at z_lo / z_hi of a scalar field [z][y][x] (channel 0, may be NULL) and of
 * the `planes` planes of a planar vector field (channels 1.., may be NULL) into (unpack = 0) or out of (unpack = 1) the
 * contiguous messages msg_lo / msg_hi (each [1 + planes][halo][ny][nx] floats; NULL = no neighbour on that side). */
int lsf_halo_copy(float *scalar, float *planar, float *msg_lo, float *msg_hi, const lsf_grid *grid, int32_t planes,
                  int32_t halo, int32_t z_lo, int32_t z_hi, int32_t unpack, void *stream);

/* ---- a1/a2: resample a scalar field under a warp ---------------------------------------------------
 * replaces nonrigid_opt/field_warping.py:67-85 (warp_field, oob_value = 1) and :88-109
 * (warp_field_replacement, oob_value = replacement) with utils/sampling.py:139-175,222-263. */
int lsf_warp_field(const float *field, const float *warp_planar, float *out, const lsf_grid *grid,
                   float oob_value, void *stream);

/* ---- a3: truncation-aware re-warp -------------------------------------------------------------------
 * replaces nonrigid_opt/field_warping.py:112-151 and the C++ twin cpp.warp_field_advanced called at
 * nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:227-228.  warp (and gradient, may be NULL) are zeroed in
 * place where the new value snaps to +-1.  flags: bit0 band_union_only, bit1 known_values_only,
 * bit2 substitute_original. */
int lsf_warp_field_advanced(const float *canonical, const float *live, float *warp_planar,
                            float *gradient_planar, float *new_live, const lsf_grid *grid, int32_t flags,
                            void *stream);

/* ---- a4 + packing: np.gradient of the live field, packed with it as float4 ------------------------
 * replaces np.gradient at hierarchical_optimizer2d.py:126 (+ the four pyramids' level-0 inputs :128-131) */
int lsf_pack_live_gradient(const float *live, float *packed4, const lsf_grid *grid, void *stream);

/* ---- a5/a6: pyramid restrict (2^D block mean, per channel) and prolong (repeat, no rescale) -------
 * replaces nonrigid_opt/hierarchical/pyramid.py:45-56 and hierarchical_optimizer2d.py:155-156.
 * `fine` describes the fine grid; the coarse grid has every extent halved (nz stays 1 in 2-D).
 * restrict: interleaved channels (1 = scalar, 4 = packed live field).  prolong: planar vector field. */
int lsf_restrict_mean(const float *fine, float *coarse, const lsf_grid *fine_grid, int32_t channels,
                      void *stream);
int lsf_prolong_repeat(const float *coarse_planar, float *fine_planar, const lsf_grid *fine_grid, void *stream);

/* LINEAR resampling strategy, 3-D only: replaces math_utils/resampling.py:29-80 (upsample2x_linear: 0.75 / 0.25
 * trilinear prolongation, edge padded) and :83-126 (downsample2x_linear: 4x4x4 window with the reference's literal
 * weights, edge padded).  `fine_grid` describes the FINE grid (even extents); interleaved channels 1 or 4. */
int lsf_upsample2x_linear(const float *coarse, float *fine, const lsf_grid *fine_grid, int32_t channels,
                          void *stream);
int lsf_downsample2x_linear(const float *fine, float *coarse, const lsf_grid *fine_grid, int32_t channels,
                            void *stream);

/* ---- a9/a10: one pass of the separable convolution along one axis (0 = x, 1 = y, 2 = z) ------------
 * replaces math_utils/convolution.py:70-111 (convolve_with_kernel) and :114-132 (…_preserve_zeros) pass by
 * pass: out[i] = sum_j k[j]*in[i + n/2 - j], zero padded, accumulated in float64 in tap order, stored
 * float32.  zero_mask_source (may be NULL): where |zero_mask_source| < 1e-6 the output is forced to 0
 * (convolution.py:118,123,127).  Operates on `planes` planes of a planar vector field. */
int lsf_convolve_axis(const float *in_planar, float *out_planar, const float *zero_mask_source,
                      const lsf_grid *grid, int32_t planes, int32_t axis, const double *taps_host,
                      int32_t n_taps, const lsf_gate *gate, void *stream);
/* the x and the y pass of a 3-D filter in one launch, without a zero mask (levels below lsf_convolve_xyz's size, where the
 * passes are launch-bound): the result equals lsf_convolve_axis along x, then along y, bit for bit, on the grid's z-range.
 * nx % 4 == 0, 3 / 5 / 7 / 9 taps (LSF_ERR_BAD_DIMS / LSF_ERR_KERNEL_TOO_LONG otherwise). */
int lsf_convolve_xy(const float *in_planar, float *out_planar, const lsf_grid *grid, int32_t planes,
                    const double *taps_host, int32_t n_taps, const lsf_gate *gate, void *stream);
/* the LAST pass of a hierarchical iteration's 3-D filter (axis 2; axis 1 is accepted too -- the reference's 2-D filter ends
 * with its x pass, convolution.py:77-83, which this does not cover; 3 / 5 / 7 / 9 taps, no zero mask): the
 * same pass, which also moves the warp by the filtered gradient it writes, component by component -- warp -= rate * out
 * (hierarchical_optimizer2d.py:220-222; what lsf_convolve_xyz does on large levels): lsf_hier_update is then called with
 * a NULL warp (the maximum only), or not at all when the next iteration takes the maximum (lsf_hier_params::previous_max).
 * LSF_ERR_BAD_DIMS for other tap counts. */
int lsf_convolve_axis_update(const float *in_planar, float *out_planar, float *warp_planar, float rate,
                             const lsf_grid *grid, int32_t planes, int32_t axis, const double *taps_host,
                             int32_t n_taps, const lsf_gate *gate, void *stream);

/* the three passes of a 3-D filter (x, then y, then z: convolution.py:94-105) in one launch, without a zero mask: the
 * result equals three lsf_convolve_axis calls bit for bit (x and y passes on every slice the z pass reads, z pass on the
 * grid's z-range: a z-slab filters its owned slices from raw input whose halo slices are valid).  nx % 4 == 0,
 * 3 / 5 / 7 / 9 taps; LSF_ERR_BAD_DIMS / LSF_ERR_KERNEL_TOO_LONG otherwise (the caller then runs the single passes).
 * warp_planar (may be NULL): the filtered field also moves the warp, warp -= rate * out, component by component -- the
 * hierarchical optimizer's update (hierarchical_optimizer2d.py:220-221) without another pass over out; the caller
 * then calls lsf_hier_update with warp_planar = NULL for the record's maximum. */
int lsf_convolve_xyz(const float *in_planar, float *out_planar, float *warp_planar, float rate, const lsf_grid *grid,
                     int32_t planes, const double *taps_host, int32_t n_taps, const lsf_gate *gate, void *stream);

/* the same zero-preserving pass (zero_mask_source required, 3 / 5 / 7 / 9 taps) at the voxels of a band list only */
int lsf_convolve_axis_listed(const float *in_planar, float *out_planar, const float *zero_mask_source,
                             const lsf_grid *grid, int32_t planes, int32_t axis, const double *taps_host,
                             int32_t n_taps, const lsf_gate *gate, const int32_t *band_list, int64_t band_count,
                             void *stream);

/* ---- hierarchical optimizer iteration ---------------------------------------------------------------
 * replaces one pass of the loop body nonrigid_opt/hierarchical/hierarchical_optimizer2d.py:184-225:
 *   resample live and its gradients under `warp` (a1,a2), data term (a7), Tikhonov = Laplacian of the
 *   previous gradient (a8), and -- when apply_update != 0 (no gradient kernel) -- warp -= rate*g and the
 *   max-update reduction (a11).  With a gradient kernel the caller runs lsf_convolve_axis passes on
 *   g_out and then lsf_hier_update.
 * gate (may be NULL): see lsf_gate.  g_prev_planar may be NULL when Tikhonov is off; g_out_planar may be NULL
 * when apply_update is set and the gradient is not wanted. */
typedef struct lsf_hier_params {
    float data_term_amplifier;
    float tikhonov_strength;   /* used when tikhonov_enabled */
    float rate;
    int32_t tikhonov_enabled;
    int32_t apply_update;
    int32_t compute_energy;    /* accumulate sum(diff^2) into the record's data_energy */
    int32_t previous_max;      /* 3-D, Tikhonov on, apply_update off, gate->prev_record set: ALSO write the maximum length
                                  (and arg-max) of g_prev -- the previous iteration's final gradient, which this kernel
                                  reads anyway -- into gate->prev_record.  For runs whose stop test cannot fire
                                  (threshold <= 0): the maximum is then only a log value and needs no pass of its own
                                  (lsf_hier_update with a NULL warp) except after the last iteration. */
    int32_t reserved;
    /* z-slab runs (3-D): the packed live field -- the only operand read through the data-dependent gather -- may hold MORE
     * slices than the grid: packed_nz > 0 says how many, packed_z_global_offset the global z of its slice 0 (0 for a copy
     * of the whole level replicated on every rank, SURVEY 8e: the gather then never leaves the device however far the
     * cumulative warp reaches).  packed_nz == 0: the packed field has the grid's own extent and offset. */
    int32_t packed_nz;
    int32_t packed_z_global_offset;
} lsf_hier_params;

int lsf_hier_iteration(const float *packed_live4, const float *canonical, float *warp_planar,
                       const float *g_prev_planar, float *g_out_planar, const lsf_grid *grid,
                       const lsf_hier_params *params, const lsf_gate *gate, lsf_iteration_record *record,
                       void *stream);

/* warp -= rate*g ; the record's max_packed = max |g|   (hierarchical_optimizer2d.py:220-225).  warp_planar may be
 * NULL: only the maximum (the warp was moved by lsf_convolve_xyz already). */
/* A whole 2-D level, K = iterations_per_launch (1..8) iterations per launch: temporal blocking through LDS (round 6;
 * BASELINE config 2 is launch-bound -- a 512^2 level is 1024 voxels per CU).  Replaces `iterations` calls of
 * lsf_hier_iteration (Tikhonov term, apply_update = 1, no energies; hierarchical_optimizer2d.py:184-225) with
 * ceil(iterations / K) launches whose workgroups each advance a 32 x 32 tile K iterations inside LDS, recomputing the
 * K - 1 - j rings of voxels around it that iteration j needs (identical arithmetic on identical inputs: identical results).
 * Launch b reads (warp_a, g_a) when b is even, (warp_b, g_b) when odd, and writes the other pair.  records[0..iterations):
 * one record per iteration (the caller has zeroed them), maxima only.
 * threshold <= 0 (the stop test cannot fire): after the call the warp and the last iteration's gradient are in the _a
 * buffers when ceil(iterations / K) is even, in the _b buffers otherwise.
 * threshold > 0 (hierarchical_optimizer2d.py:169-171: an iteration whose maximum is below it is the level's last): launch
 * b > 0 first looks at the K records of launch b - 1 and does nothing when one of them is below the threshold or empty.  The
 * launch in which the level converged is then the last to have written anything and its input pair is intact: the caller
 * reads the records, finds the first iteration j below the threshold and, unless j is its launch's last iteration, calls
 * again with that launch's input pair as (_a), its output pair as (_b), iterations = j + 1 - b K and threshold = 0.
 * With a gradient kernel (taps_host / n_taps = 3, 5, 7 or 9; NULL / 0: none; hierarchical_optimizer2d.py:213-216): the
 * launch also runs the filter's y and x passes (convolution.py:77-83) and the update behind them -- what lsf_hier_iteration
 * with apply_update = 0, two lsf_convolve_axis passes and lsf_hier_update do in four launches; params->apply_update must
 * then be 0 as it is for those.  An iteration consumes n_taps / 2 + 1 rings of the tile's surroundings instead of one:
 * iterations_per_launch * (n_taps / 2 + 1) <= 8 (two iterations per launch for seven taps), LSF_ERR_BAD_ARGUMENT otherwise.
 * Without the Tikhonov term (tikhonov_enabled = 0) a voxel's update depends on nothing around it but through the filter:
 * iterations_per_launch * (tikhonov_enabled + n_taps / 2) <= 8 in general.
 * LSF_ERR_BAD_DIMS for anything but dims = 2, compute_energy = 0, apply_update = (n_taps == 0). */
int lsf_hier_level_run_2d(const float *packed_live4, const float *canonical, float *warp_a, float *warp_b, float *g_a,
                          float *g_b, const lsf_grid *grid, const lsf_hier_params *params, const double *taps_host,
                          int32_t n_taps, lsf_iteration_record *records, int32_t iterations,
                          int32_t iterations_per_launch, float threshold, void *stream);
int lsf_hier_update(const float *g_planar, float *warp_planar, const lsf_grid *grid, float rate,
                    const lsf_gate *gate, lsf_iteration_record *record, void *stream);

/* ---- Slavcheva (KillingFusion / SobolevFusion) optimizer iteration ----------------------------------
 * replaces nonrigid_opt/slavcheva/slavcheva_optimizer2d.py:163-236 (VECTORIZED) and :238-330 (DIRECT)
 * with data_term.py:169-227,334-358, smoothing_term.py:50-177, level_set_term.py:28-64.
 *
 * No Sobolev filter: lsf_slavcheva_state_iteration -- ONE kernel does gradient, warp = -g*rate, max-warp reduction,
 *   energies and the truncation-aware re-warp of the live field (a12-a18 + a3): the "fused per-voxel warp-update
 *   kernel", on the float4 state layout.
 * With a Sobolev filter: lsf_slavcheva_gradient (gradient + energies into g_out), lsf_convolve_axis passes
 *   (zero-preserving), lsf_slavcheva_update_rewarp -- planar fields. */
#define LSF_SMOOTHING_TIKHONOV 0
#define LSF_SMOOTHING_KILLING 1
#define LSF_DATA_BASIC 0
#define LSF_DATA_THRESHOLDED_FDM 2
#define LSF_ENERGY_NONE 0
#define LSF_ENERGY_DIRECT 1     /* per-voxel energies of DIRECT mode */
#define LSF_ENERGY_VECTORIZED 2 /* np.gradient-based smoothing energy of VECTORIZED mode */

typedef struct lsf_slavcheva_params {
    double isomorphic_enforcement_factor_f64; /* lambda as given (energies are accumulated in double) */
    float rate;
    float data_term_weight;
    float smoothing_term_weight;
    float level_set_term_weight;
    float isomorphic_enforcement_factor; /* float32(lambda) */
    float killing_c1;                    /* float32(-2*(1+lambda)), evaluated in double on the host */
    int32_t smoothing_method;
    int32_t data_method;
    int32_t level_set_enabled;
    int32_t energy_mode;
    int32_t zero_gradient_on_snap; /* DIRECT: 1 (field_warping.py:141) ; VECTORIZED: 0 */
    int32_t reserved;
} lsf_slavcheva_params;

/* band_list (may be NULL = every voxel of the z-range; LSF_BAND_ALL lists only): the SobolevFusion path on a band list --
 * gradient, the masked filter passes (lsf_convolve_axis_listed) and the update touch listed voxels only; the caller
 * zero-initialises the gradient / filter buffers and initialises BOTH ping-pong (live, warp) sets with (live, 0): a
 * zero-preserving filter cannot move gradient out of the band, so every other voxel keeps those values. */
int lsf_slavcheva_gradient(const float *live, const float *canonical, const float *warp_prev_planar,
                           float *g_out_planar, const lsf_grid *grid, const lsf_slavcheva_params *params,
                           const lsf_gate *gate, lsf_iteration_record *record, const int32_t *band_list,
                           int64_t band_count, void *stream);

/* Band lists for lsf_slavcheva_state_iteration: only listed voxels are visited.  This is exact, not an approximation:
 * a voxel outside the narrow-band union (|live| == |canonical| == 1, the test of slavcheva_optimizer2d.py:251-252 /
 * tsdf_set_routines.py:19-52) gets a zero gradient, hence warp 0 and live' = live, and so stays outside for the rest of
 * the optimisation.  The caller keeps canonical and params unchanged while a list is in use.  Records, live and warp
 * are identical with and without a list. */
#define LSF_BAND_ALL 0      /* every voxel of the narrow-band union */
#define LSF_BAND_INTERIOR 1 /* ... whose whole 3^D neighbourhood lies inside the (allocated) array */
#define LSF_BAND_BOUNDARY 2 /* ... the others (voxels on a face of the array) */

/* Band list of the grid's z-range [z_begin, z_end): the voxels with |live| != 1 or |canonical| != 1
 * (tsdf_set_routines.py:19-52; the `continue` of slavcheva_optimizer2d.py:251-252), in ascending index order --
 * all of them, or split into INTERIOR and BOUNDARY voxels.  An INTERIOR list lets lsf_slavcheva_state_iteration run a
 * kernel that never applies the reference's out-of-bounds rules (none can fire) and addresses all neighbours from one
 * per-lane offset; it requires 16 * nz * ny * nx < 2^32 (32-bit buffer offsets; LSF_ERR_BAD_ARGUMENT otherwise).
 * One iteration = one launch per non-empty list, all on the same record.
 *   1. lsf_band_count     counts per 1024-voxel chunk into scratch (lsf_band_scratch_elements(grid) int32 elements),
 *                         scans them, and writes the total to *count_out (device memory);
 *   2. the caller reads the total and allocates the list;
 *   3. lsf_band_list_fill writes the indices (same live / canonical / grid / subset / scratch as step 1). */
int64_t lsf_band_scratch_elements(const lsf_grid *grid);
int lsf_band_count(const float *live, const float *canonical, const lsf_grid *grid, int32_t subset,
                   int32_t *scratch, int64_t *count_out, void *stream);
int lsf_band_list_fill(const float *live, const float *canonical, const lsf_grid *grid, int32_t subset,
                       const int32_t *scratch, int32_t *list, void *stream);

/* ---- the fused iteration on the STATE layout (what the optimizers run when no Sobolev filter is configured) --------
 * state: float4 [z][y][x] = (live, u, v, w) (w = 0 in 2-D) -- the live field and the per-iteration warp travel together:
 * an iteration reads both through the same 3^D neighbourhood and writes both, so one 16-byte access replaces four
 * dword accesses to four planes.  band_list (may be NULL = every voxel of the z-range): ascending
 * voxel indices (z * ny + y) * nx + x from lsf_band_list_fill, band_count of them, band_subset the LSF_BAND_* it was
 * built with; state_out of BOTH ping-pong states must hold (live, 0) at unlisted voxels (lsf_state_pack with two
 * destinations does exactly that).  An INTERIOR list requires 16 * nz * ny * nx < 2^32.
 * lsf_state_pack: (live, warp planar or NULL = 0) -> state_a and, if not NULL, state_b, slices [z_begin, z_end).
 * lsf_state_unpack: state -> live and / or planar warp [c][z][y][x] and / or interleaved warp [z][y][x][c]. */
/* lsf_state_prepare: the start of an optimize() call in one pass over WHOLE arrays (z_begin = 0, z_end = nz): both
 * ping-pong states = (live, 0) (state_b may be NULL: the caller then writes it with lsf_state_pack behind its copy of
 * counts_out, where it overlaps the host's wait) and the counting step of lsf_band_count for the INTERIOR and the
 * BOUNDARY subset at once.
 * scratch: lsf_state_prepare_scratch_elements(grid) int32 (8-byte aligned); counts_out[0..4) (device) = INTERIOR and
 * BOUNDARY totals, then the number of voxels OUTSIDE the band with live = -canonical and the first of them (-1: none)
 * -- what lsf_state_finalize_listed needs to know about the voxels no list holds.  lsf_band_list_fill_prepared then writes one subset's list from the ballots the prepare pass kept
 * in scratch (16 bytes per 64 voxels) -- live and canonical are not read again.
 * state_a AND state_b NULL: the pass only counts; lsf_state_pack_needed then writes the two states (live, 0) ONLY where
 * an iteration can read them: the groups of 32 consecutive voxels that have a voxel within `reach` voxels (per axis) of a
 * band voxel -- 3^D stencils reach 1, the re-warp gather of an update shorter than `reach` voxels reaches `reach`
 * (1 <= reach <= 8).  Everything else of the two buffers stays UNINITIALISED: a run is valid only while every
 * iteration's maximum update stays below `reach` (lsf_state_finalize_listed's guard_records check that on the device,
 * the host on the records it reads), and whole-state readers (lsf_state_unpack, lsf_state_finalize) must first complete the state with
 * invert = 1 (writes exactly the groups the first call left out, from the verdicts it kept in scratch: a bit per group,
 * an int32 per 1024 voxels).  On a narrow band this replaces 2 x 16 B per VOXEL of initialisation by 2 x 16 B per voxel
 * NEAR THE BAND (a fifth of a 256^3 sphere pair).  Arrays of fewer than 2^21 voxels (LSF_SPARSE_MIN_VOXELS in the
 * environment moves the limit) keep whole 1024-voxel chunks: a chunk near a chunk with band voxels is written whole and
 * its kept word is 1. */
int64_t lsf_state_prepare_scratch_elements(const lsf_grid *grid);
int lsf_state_pack_needed(const float *live, float *state_a, float *state_b, const lsf_grid *grid, int32_t *scratch,
                          int32_t reach, int32_t invert, void *stream);

int lsf_band_list_fill_prepared(const lsf_grid *grid, int32_t subset, const int32_t *scratch, int32_t *list,
                                void *stream);
int lsf_state_prepare(const float *live, const float *canonical, float *state_a, float *state_b,
                      const lsf_grid *grid, int32_t *scratch, int64_t *counts_out, void *stream);
int lsf_state_pack(const float *live, const float *warp_planar, float *state_a, float *state_b,
                   const lsf_grid *grid, void *stream);
int lsf_state_unpack(const float *state, float *live_out, float *warp_planar_out, float *warp_interleaved_out,
                     const lsf_grid *grid, void *stream);
/* end of an optimize() call in one pass over slices [z_begin, z_end): state -> live_out, planar and / or interleaved warp
 * (each may be NULL) and -- when statistics16 is not NULL -- the convergence statistics of
 * lsf_warp_statistics (statistics16[0..8)) and lsf_tsdf_difference_statistics (statistics16[8..16)) of the final
 * fields (a20; cpp.build_warp_delta_statistics_2d / build_tsdf_difference_statistics_2d, slavcheva_optimizer2d.py:394-398).
 * scratch: lsf_state_finalize_scratch_elements(grid) doubles of device memory. */
int64_t lsf_state_finalize_scratch_elements(const lsf_grid *grid);
int lsf_state_finalize(const float *state, const float *canonical, float *live_out, float *warp_planar_out,
                       float *warp_interleaved_out, const lsf_grid *grid, float lower_threshold,
                       double *statistics16, double *scratch, void *stream);
/* the same pass for final fields that are planar (the SobolevFusion path: live [z,]y,x and warp [c][z,]y,x): live_out
 * (may be NULL, must not be live), the interleaved warp and the statistics in one pass instead of a copy, an interleave
 * and the two statistics kernels.  scratch as lsf_state_finalize. */
int lsf_planar_finalize(const float *live, const float *warp_planar, const float *canonical, float *live_out,
                        float *warp_interleaved_out, const lsf_grid *grid, float lower_threshold,
                        double *statistics16, double *scratch, void *stream);

/* lsf_state_finalize for whole arrays whose band lists are at hand: only the listed voxels are visited -- live_out must
 * already hold the INPUT live field and warp_interleaved_out zeros (nothing else can have changed); the statistics
 * take the unlisted voxels from lsf_state_prepare's counts_out[2..4): opposite_count of them have
 * |canonical - live| = 2, the first one at voxel first_opposite (-1: none), the others 0.  scratch as lsf_state_finalize.
 * skip_flag (may be NULL): a DEVICE word; when it is non-zero as the pass runs, live_out and warp_interleaved_out are
 * left untouched (and the statistics are meaningless) -- the chain add-on (include/lsf_hip_chain.h) raises such a word.
 * guard_records (may be NULL): the pass also leaves everything untouched when one of guard_records[0..guard_count) was
 * executed with a maximum update that is not below guard_limit (NaN included): the run's sparsely initialised states
 * (lsf_state_pack_needed) may then have been read where they were never written. */
int lsf_state_finalize_listed(const float *state, const float *canonical, float *live_out, float *warp_interleaved_out,
                              const lsf_grid *grid, const int32_t *const *band_lists, const int64_t *band_counts,
                              int32_t n_lists, int64_t opposite_count, int64_t first_opposite, float lower_threshold,
                              double *statistics16, double *scratch, const int32_t *skip_flag,
                              const lsf_iteration_record *guard_records, int32_t guard_count, float guard_limit,
                              void *stream);
int lsf_slavcheva_state_iteration(const float *state_in, const float *canonical, float *state_out,
                                  const lsf_grid *grid, const lsf_slavcheva_params *params, const lsf_gate *gate,
                                  lsf_iteration_record *record, const int32_t *band_list, int64_t band_count,
                                  int32_t band_subset, void *stream);

/* ---- the cumulative warp of a call on the state layout ("Cumulative warp") -----------------------
 * Every iteration re-warps the live field by its own update, live_{k+1}(v) = live_k(v + u_k(v)), so the call's total
 * displacement PSI with live_0(v + PSI(v)) ~ canonical(v) is the composition PSI_0 = 0, PSI_{k+1}(v) = u_k(v) +
 * PSI_k(v + u_k(v)).  lsf_cumulative_warp_compose is one step of it, launched behind the iteration whose output state it
 * reads.  The rule, D = 2 and 3, for every listed voxel v and component c, with u the update `state` holds at v (the
 * post-snap update: zero where the re-warped live value snapped to +-1):
 *     psi_out_c(v) = float32( u_c(v) + S_c ),   S_c = sample_linear(psi_in_c, position(v, u), oob = 0)
 * position(v, u) = float32(coordinate) + u per axis in float32 (z from the GLOBAL coordinate, z + z_global_offset);
 * sample_linear lerps z, then y, then x, every tap outside the array reads 0, multiply and add rounded separately;
 * positions are clamped before the integer conversion, so a non-finite or huge update addresses valid cells only.
 * Outside the band u = 0 and PSI stays 0: only listed voxels are written, psi_in AND psi_out must hold zeros at every
 * unlisted voxel (two zero-filled buffers, ping-pong).  An iteration the gate skips composes nothing: `gate` is the gate
 * of the iteration this launch follows (both read record i - 1 and decide alike); min_iterations == 0 leaves PSI = 0.
 * state, psi_in, psi_out: float4 [z][y][x], 16-byte aligned, psi = (unused, x, y, z) in the state's channel order, so
 * lsf_state_unpack(psi, NULL, NULL, interleaved) gives the API layout [z][y][x][c].  psi_in, psi_out and state must not
 * overlap.  band_list (NULL = every voxel of the z-range, band_count 0) / band_count (> 0 with a list) as
 * lsf_slavcheva_state_iteration, any subset.  One launch, no host synchronisation, no atomics, no record.
 * Refused before any launch, all with LSF_ERR_BAD_ARGUMENT: a NULL buffer, a base off 16-byte alignment, psi_in ==
 * psi_out or any overlap among state, psi_in and psi_out, a grid with bad dims, extents or z range or cut along y, a
 * negative band_count or one past int32, a list with band_count <= 0, a band_count without a list. */
int lsf_cumulative_warp_compose(const float *state, const float *psi_in, float *psi_out, const lsf_grid *grid,
                                const lsf_gate *gate, const int32_t *band_list, int64_t band_count, void *stream);

/* ---- the fused iteration over BOXES (3-D, INTERIOR band voxels) -----------------------------
 * The same pass of slavcheva_optimizer2d.py:238-330 as lsf_slavcheva_state_iteration over an INTERIOR band list, same
 * results, with the work cut differently: a box is 4 x 4 x 4 voxels whose lowest corner (x0, y0, z0) has coordinates that
 * are multiples of 4 -- origin = (z0 * ny + y0) * nx + x0 --, bit (lz * 4 + ly) * 4 + lx of `mask` says whether voxel
 * (x0 + lx, y0 + ly, z0 + lz) is an INTERIOR band voxel (LSF_BAND_INTERIOR: its whole 3^3 neighbourhood inside the array).
 * Boxes in ascending order of origin, every INTERIOR band voxel in exactly one box; voxels on the faces of the array keep
 * their BOUNDARY list and lsf_slavcheva_state_iteration.  A wave stages a box and its one-voxel shell through LDS instead
 * of loading 18 neighbours per voxel.  Requires dims = 3, extents that are multiples of 4, nz * ny * nx < 2^28
 * (LSF_ERR_BAD_DIMS otherwise).  lsf_band_boxes_count / _fill build the boxes from the ballots lsf_state_prepare kept in its
 * scratch: _count writes the number of boxes to *count_out (device) and keeps per-group counts in box_scratch
 * (lsf_band_boxes_scratch_elements(grid) int32), the caller reads the count, allocates, and _fill writes the boxes. */
typedef struct lsf_band_box {
    int32_t origin;
    int32_t reserved;
    uint64_t mask;
} lsf_band_box;
int64_t lsf_band_boxes_scratch_elements(const lsf_grid *grid);
/* subset: LSF_BAND_INTERIOR (the boxes of lsf_slavcheva_state_iteration_boxes) or LSF_BAND_ALL (every band voxel, those on
 * the faces included: lsf_sobolev_state_update_boxes); the same value in both calls */
int lsf_band_boxes_count(const lsf_grid *grid, int32_t subset, const int32_t *prepare_scratch, int32_t *box_scratch,
                         int64_t *count_out, void *stream);
int lsf_band_boxes_fill(const lsf_grid *grid, int32_t subset, const int32_t *prepare_scratch, const int32_t *box_scratch,
                        lsf_band_box *boxes, void *stream);
/* the canonical values of the boxes' voxels, box by box: canonical_boxed[64 b + (lz * 4 + ly) * 4 + lx] -- what the box walk
 * reads instead of the [z][y][x] array (256 contiguous bytes per box instead of sixteen rows of 16 bytes); once per call */
int lsf_band_boxes_canonical(const float *canonical, const lsf_grid *grid, const lsf_band_box *boxes, int64_t box_count,
                             float *canonical_boxed, void *stream);
int lsf_slavcheva_state_iteration_boxes(const float *state_in, const float *canonical_boxed, float *state_out,
                                        const lsf_grid *grid, const lsf_slavcheva_params *params, const lsf_gate *gate,
                                        lsf_iteration_record *record, const lsf_band_box *boxes, int64_t box_count,
                                        void *stream);

/* ---- a whole fixed-count call of the fused path, enqueued by the library in two host calls ---------------------------
 * replaces the LOOP of slavcheva_optimizer2d.py:354-388 (min_iterations == max_iterations: its stop test :360-362 cannot
 * fire) around the calls above, for whole volumes on band lists: lsf_state_run_begin launches lsf_state_prepare and the
 * initialisation of the two states (sparse_reach > 0: lsf_state_pack_needed with that reach, else both states in full,
 * the second one behind the copy of the list sizes when second_state_late != 0) and RETURNS when the four totals of
 * lsf_state_prepare are in totals_host; the caller sizes the two lists from them (totals_host[0] INTERIOR, [1] BOUNDARY
 * entries) and calls lsf_state_run_finish, which launches the list fills, `iterations` x lsf_slavcheva_state_iteration
 * per non-empty list (ungated; iteration i reads state[i % 2], writes the other, reduces into records[i], which the
 * caller has zeroed; with `boxes` -- room for totals_host[4] of them, box_scratch given to lsf_state_run_begin, and
 * `box_canonical`, room for 64 floats per box -- the INTERIOR voxels are walked box by box instead,
 * lsf_band_boxes_canonical + lsf_slavcheva_state_iteration_boxes: same results) and lsf_state_finalize_listed of the final state into live_out (which must hold the input live field:
 * the pass writes listed voxels only; statistics16 / finalize_scratch as there, may be NULL; with sparse states the pass
 * guards itself with the records), copies the records' used words and the statistics to the host in ONE transfer and
 * RETURNS when the stream has drained, the records decoded into `result` (lsf_records_decode).  The same launches in the
 * same order as the calls made one by one: identical results.  Both functions block the calling thread only (no
 * device-wide synchronisation); totals_host and words_host must be page-locked host memory; words_host and words_device
 * hold iterations x LSF_RECORD_SLOTS x 4 + 16 int64: the used words of every record slot, then the 16 statistics (as
 * doubles; zeros without statistics16).
 * Threshold-terminated calls (round 6; `loop` not NULL and min_iterations < max_iterations: every reference caller's
 * default, slavcheva_optimizer2d.py:360-362 -- min 1, max 100, lower threshold 0.1): `iterations` = max_iterations is the
 * number of records; iteration i >= min_iterations is launched behind the device-side gate on record i - 1 (lsf_gate,
 * LSF_GATE_SLAVCHEVA with the two thresholds), `check_interval` iterations at a time; after each batch the function reads
 * the batch's records (one small transfer, one wait) and stops enqueueing when the reference's loop would have ended --
 * so the executed count, every record and the final fields are the reference's, and at most check_interval - 1 gated
 * no-op launches are wasted.  The finalize pass then reads state[executed % 2]. */
typedef struct lsf_run_loop {
    int32_t min_iterations;  /* >= 1 (with 0 the reference never enters its loop: the caller handles that) */
    int32_t max_iterations;  /* the loop runs while it < min or (it < max and lower < max_warp < upper) */
    float lower_threshold, upper_threshold;
    int32_t check_interval;  /* >= 1 */
    int32_t reserved;
} lsf_run_loop;
typedef struct lsf_state_run {
    const float *live;        /* the input live field; read again by the sparse initialisation */
    const float *canonical;
    float *state[2];          /* the two ping-pong states, nz * ny * nx float4 each, contents undefined on entry */
    int32_t *prepare_scratch; /* lsf_state_prepare_scratch_elements(grid) int32 */
    int64_t *totals_device;   /* 5 int64 */
    int64_t *totals_host;     /* 5 int64, page-locked: lsf_state_prepare's four totals, then the number of boxes (or 0) */
    lsf_grid grid;            /* a whole volume: z_begin = 0, z_end = nz, no offsets */
    int32_t sparse_reach;     /* 0: both states are written in full */
    int32_t second_state_late;
    int32_t *box_scratch;     /* NULL, or lsf_band_boxes_scratch_elements(grid) int32: lsf_state_run_begin then also counts the
                                 boxes of lsf_slavcheva_state_iteration_boxes (totals_host[4]) */
    int32_t box_all;          /* 0: the boxes of the INTERIOR band voxels (lsf_state_run_finish); 1: of ALL band voxels
                                 (LSF_BAND_ALL: lsf_sobolev_run_finish) */
    int32_t reserved;
} lsf_state_run;
typedef struct lsf_state_run_result {
    float *max_value;    /* host arrays of `iterations` entries (energies3: 3 per iteration), as lsf_records_decode */
    int64_t *argmax;
    double *energies3;
    uint8_t *executed;
    int32_t final_state;    /* out: index of the state that holds the result (iterations % 2) */
    int32_t n_lists;        /* out: launches per iteration */
    int32_t reach_exceeded; /* out: sparse states and an update of sparse_reach voxels or more -- live_out was left alone
                               (the finalize pass's guard) and the call has to be repeated on full states */
    int32_t compact_faces;  /* out (lsf_slab_run_finish): 1 = only the band voxels of the faces travelled, 0 = whole slices
                               (no message buffer given, or a neighbour's face counts disagreed), -1 = nothing was exchanged */
} lsf_state_run_result;
int lsf_state_run_begin(const lsf_state_run *run, void *stream);
int lsf_state_run_finish(const lsf_state_run *run, const lsf_slavcheva_params *params, int32_t *list_interior,
                         int32_t *list_boundary, lsf_band_box *boxes, float *box_canonical, lsf_iteration_record *records,
                         int32_t iterations, const lsf_run_loop *loop /* NULL: `iterations` ungated launches */,
                         float *live_out,
                         float lower_threshold, double *statistics16, double *finalize_scratch, int64_t *words_device,
                         int64_t *words_host, lsf_state_run_result *result, void *stream);
/* lsf_state_run_finish with RECORD ROWS.  No launch of a fixed-count call (loop NULL, or min_iterations >= iterations) reads
 * a record, so with a rows buffer its iteration launches end without the workgroup-wide reduction and the atomics: every
 * wave stores one row {max_packed, three energy sums} of 4 int64, and ONE launch behind the last iteration (one workgroup
 * per iteration, a fixed association: the same bits on every run) combines each iteration's rows into slot 0 of its record
 * and zeroes the other slots' used words -- the finalize pass's guard, words_host and `result` are what
 * lsf_state_run_finish gives, the energies to the rounding of another order of float64 adds.  record_rows: DEVICE memory,
 * 32-byte aligned, contents undefined on entry, record_rows_elements >= lsf_state_run_rows_elements(&run->grid, iterations,
 * launches per iteration) int64 or the call is refused before it launches anything; NULL: lsf_state_run_finish.  A call
 * whose stop test can fire keeps the atomics (the next launch's gate and the host read its records between launches) and
 * leaves the buffer alone.  *rows_taken (may be NULL): 1 when the launches ended in rows, else 0. */
int lsf_state_run_finish_rows(const lsf_state_run *run, const lsf_slavcheva_params *params, int32_t *list_interior,
                              int32_t *list_boundary, lsf_band_box *boxes, float *box_canonical,
                              lsf_iteration_record *records, int32_t iterations, const lsf_run_loop *loop, float *live_out,
                              float lower_threshold, double *statistics16, double *finalize_scratch, int64_t *words_device,
                              int64_t *words_host, lsf_state_run_result *result, int64_t *record_rows,
                              int64_t record_rows_elements, int32_t *rows_taken, void *stream);
/* int64 elements of record_rows for `iterations` iterations of n_lists launches each (1, or 2 when totals_host[0] and [1] are
 * both non-zero) on this grid, whatever the lists' lengths: the launchers' own largest grids, one row per wave; 0 for
 * arguments that make no call. */
int64_t lsf_state_run_rows_elements(const lsf_grid *grid, int32_t iterations, int32_t n_lists);

/* The SobolevFusion counterpart of lsf_state_run_finish (round 6): the loop of slavcheva_optimizer2d.py:354-388 WITH a Sobolev
 * filter, for whole 3-D volumes of whole boxes (the conditions of lsf_sobolev_state_update_boxes), behind a
 * lsf_state_run_begin with box_scratch and box_all = 1.  Launches the list fills, the ascending list of ALL band voxels
 * (lsf_merge_sorted_runs into list_all -- room for totals_host[0] + totals_host[1] entries -- when both lists have entries),
 * the boxes (room for totals_host[4]), then per iteration lsf_sobolev_state_gradient_x (bricks) into g4_a and
 * lsf_sobolev_state_update_boxes (the final gradient into g4_b: in the last iteration of a fixed count, in every iteration
 * of a threshold-terminated call), the listed finalize pass and the read-backs; `loop`, records, words, result as
 * lsf_state_run_finish.  g4_a / g4_b: nz * ny * nx float4 each, ZERO-filled by the caller.  Same launches in the same order as
 * the calls made one by one: identical results. */
int lsf_sobolev_run_finish(const lsf_state_run *run, const lsf_slavcheva_params *params, const double *taps_host,
                           int32_t n_taps, int32_t *list_interior, int32_t *list_boundary, int32_t *list_all,
                           lsf_band_box *boxes, float *g4_a, float *g4_b, lsf_iteration_record *records, int32_t iterations,
                           const lsf_run_loop *loop, float *live_out, float lower_threshold, double *statistics16,
                           double *finalize_scratch, int64_t *words_device, int64_t *words_host,
                           lsf_state_run_result *result, void *stream);

/* ---- the SobolevFusion iteration on the float4 layouts (band lists) ------------------------------
 * replaces one pass of slavcheva_optimizer2d.py:163-236 / :238-330 WITH a Sobolev filter (math_utils/convolution.py:
 * 114-132) exactly as lsf_slavcheva_gradient + lsf_convolve_axis_listed x D + lsf_slavcheva_update_rewarp do on planar
 * fields -- same results -- with one vector-memory instruction per neighbour / tap instead of one per component:
 *   state  float4 [z][y][x] = (live, u, v, w)        as lsf_slavcheva_state_iteration (two ping-pong copies, both
 *                                                    (live, 0) at unlisted voxels: lsf_state_prepare / lsf_state_pack)
 *   g4     float4 [z][y][x] = (g_x, g_y, g_z, m)     raw gradient (m = 0), filter intermediates (m = mask bits 1 | 2 | 4 of the
 *                                                    three components, 8: a listed voxel), final gradient (m = 0); the caller
 *                                                    zero-initialises them once (unlisted voxels are never written)
 * One iteration = lsf_sobolev_state_gradient, lsf_convolve_axis_listed4 for every axis but the last (3-D: x, y; 2-D: y),
 * lsf_sobolev_state_update for the last (3-D: z, 2-D: x) -- each once per band list (ascending voxel indices of any
 * LSF_BAND_* subset; first_list != 0 on the call that stands for the unlisted voxels' zero update in the arg-max).
 * 3 / 5 / 7 / 9 taps (LSF_ERR_KERNEL_TOO_LONG otherwise); 16 * nz * ny * nx need not fit 32 bits.
 * zero_mask_source4: the RAW gradient for the FIRST pass (its own input: math_utils/convolution.py:118 computes the mask
 * before filtering) -- that pass leaves the three verdicts as bits in the fourth component of out4 --, NULL for every
 * later pass (and for lsf_sobolev_state_update behind at least one pass): the mask is then read from the fourth
 * component of in4's centre tap and handed on, one 16-byte load per voxel and pass less. */
int lsf_sobolev_state_gradient(const float *state, const float *canonical, float *g_raw4, const lsf_grid *grid,
                               const lsf_slavcheva_params *params, const lsf_gate *gate, lsf_iteration_record *record,
                               const int32_t *band_list, int64_t band_count, void *stream);
/* 3-D: lsf_sobolev_state_gradient and the x pass (the FIRST pass of a volume, math_utils/convolution.py:94-105) in ONE
 * launch: out4 = what lsf_convolve_axis_listed4(raw, out4, raw, axis 0) would hold, bit for bit, mask bits included; the
 * raw gradient is never stored.  band_list must then hold EVERY band voxel whose gradient can be non-zero (one
 * ascending list of the whole band, e.g. LSF_BAND_ALL): a tap at a voxel that is not in THIS list counts as zero.
 * out_bricks != 0 (extents that are multiples of 4: LSF_ERR_BAD_DIMS otherwise): out4 is laid out in BRICKS of 4 x 4 x 4
 * voxels, 1 KB each -- voxel (x, y, z) at float4 index (((z/4 * ny/4 + y/4) * nx/4 + x/4) * 64 + (z%4 * 4 + y%4) * 4 + x%4)
 * --, the layout lsf_sobolev_state_update_boxes stages its footprints from (a box's footprint is then 23 contiguous pieces
 * instead of 100 rows of 64 bytes a row's pitch apart). */
int lsf_sobolev_state_gradient_x(const float *state, const float *canonical, float *out4, const lsf_grid *grid,
                                 const lsf_slavcheva_params *params, const double *taps_host, int32_t n_taps,
                                 const lsf_gate *gate, lsf_iteration_record *record, const int32_t *band_list,
                                 int64_t band_count, int32_t out_bricks, void *stream);
/* zeros at the voxels of a band list in a float4 buffer (bricks != 0: in the brick layout of lsf_sobolev_state_gradient_x): a
 * gradient buffer whose non-zero entries all lie at the voxels of a PREVIOUS call's lists is made all-zero again without a
 * fill of the whole buffer (new design: the reference allocates its gradient per call, slavcheva_optimizer2d.py:343-346) */
int lsf_zero_listed4(float *field4, const lsf_grid *grid, const int32_t *band_list, int64_t band_count, int32_t bricks,
                     void *stream);
int lsf_convolve_axis_listed4(const float *in4, float *out4, const float *zero_mask_source4, const lsf_grid *grid,
                              int32_t axis, const double *taps_host, int32_t n_taps, const lsf_gate *gate,
                              const int32_t *band_list, int64_t band_count, void *stream);
/* Walk order of the LAST pass of a volume (along z): the ascending band list regrouped strip by strip -- `strips` strips of
 * ceil(ny / strips) rows, each swept through all slices, ascending inside a strip -- so that the z -/+ taps of a workgroup
 * are lines its own XCD has just read (results do not depend on the order).  out: band_count
 * entries; scratch: 3 * n_strips * nz int32 with n_strips = ceil(ny / ceil(ny / strips)) <= strips. */
int lsf_band_list_strip_major(const int32_t *band_list, int64_t band_count, const lsf_grid *grid, int32_t strips,
                              int32_t *out, int32_t *scratch, void *stream);
/* g_out4 of lsf_sobolev_state_update may be NULL: the iteration's filtered gradient is then not stored (a caller that
 * knows which iteration is the last one -- a fixed iteration count -- only needs that one's). */
int lsf_sobolev_state_update(const float *in4, const float *zero_mask_source4, const float *state_in, float *state_out,
                             float *g_out4, const lsf_grid *grid, const lsf_slavcheva_params *params, int32_t axis,
                             const double *taps_host, int32_t n_taps, const lsf_gate *gate,
                             lsf_iteration_record *record, const int32_t *band_list, int64_t band_count,
                             int32_t first_list, void *stream);
/* 3-D whole volumes: everything behind the FIRST pass in ONE launch, box by box -- the y pass, the z pass, the update and the
 * re-warp of slavcheva_optimizer2d.py:208-236 / math_utils/convolution.py:94-132 / field_warping.py:112-151, i.e. what
 * lsf_convolve_axis_listed4(in4, tmp, NULL, axis 1) followed by lsf_sobolev_state_update(tmp, NULL, ..., axis 2, ...,
 * first_list = 1) over one list of the whole band leave in state_out, g_out4 and the record, bit for bit, without `tmp`:
 * a wave stages the x-filtered gradient of a box's filter footprint (4 x (4 + 2c) x (4 + 2c) float4, c = n_taps / 2) and
 * the state's shell of the box through LDS.  in4: the output of
 * lsf_sobolev_state_gradient_x with out_bricks = 1 (bit 8 of its fourth component marks a listed voxel; every other brick
 * zero); g_out4 ([z][y][x] like the states) must not be in4 (other boxes
 * still read it) and may be NULL; boxes: lsf_band_boxes_count / _fill with LSF_BAND_ALL.  Requires dims = 3, extents that
 * are multiples of 4, the whole array as launch range, nz * ny * nx < 2^27 (LSF_ERR_BAD_DIMS otherwise). */
int lsf_sobolev_state_update_boxes(const float *in4, const float *state_in, float *state_out, float *g_out4,
                                   const lsf_grid *grid, const lsf_slavcheva_params *params, const double *taps_host,
                                   int32_t n_taps, const lsf_gate *gate, lsf_iteration_record *record,
                                   const lsf_band_box *boxes, int64_t box_count, void *stream);

/* ---- z-slab runtime of the fused path for multi-GPU runs (new design) -----------------------------
 * One process per GPU; rank r owns z-slices [z_begin, z_end) of its local array and keeps `halo` slices of its
 * neighbours on either interior side.  lsf_slab_state_iteration enqueues ONE whole iteration with one host call:
 *   1. lsf_slavcheva_state_iteration over the boundary parts (the `halo` owned slices next to each neighbour),
 *   2. the exchange of those slices of state_out with the neighbours -- ncclSend / ncclRecv in one group on the
 *      communicator's own HIP stream (RCCL over xGMI), each face one contiguous run of halo * ny * nx float4 --
 *   3. while the interior parts run on `stream`; 4. `stream` then waits for the halos.
 * Exchange groups: with a halo of k slices the faces need to travel only every k-th iteration when the iterations in
 * between recompute the neighbours' slices they still have valid inputs for (iteration j of a group runs over the owned
 * range widened by k - 1 - j slices, energies limited to the owned range by lsf_grid::energy_z_*; each iteration
 * consumes one slice of validity while every warp update stays below one voxel).  Those iterations pass exchange = 0.
 * RCCL is bound with dlopen (rccl_library_path, else "librccl.so" as already mapped into the process).
 * Communicator: rank 0 calls lsf_slab_unique_id, the 128 bytes travel to the other ranks by any means (the Python side
 * broadcasts them with torch.distributed), every rank calls lsf_slab_comm_create on its current device. */
#define LSF_SLAB_LAUNCH 0            /* launches only (boundary parts, then interior parts): inside an exchange group */
#define LSF_SLAB_EXCHANGE 1          /* boundary parts -> exchange || interior parts -> the stream waits for the halos */
#define LSF_SLAB_EXCHANGE_DEFERRED 2 /* the same, but the wait is left to the next call, which must be a RESUME */
#define LSF_SLAB_RESUME 3            /* "boundary" parts = what does not read the halos (runs while the previous call's
                                        exchange is in flight), wait for that exchange, then the "interior" parts */
typedef struct lsf_slab_comm lsf_slab_comm;
typedef struct lsf_slab_layout {
    int32_t nz, ny, nx;       /* local array (owned slab + halos) */
    int32_t z_begin, z_end;   /* owned slices */
    int32_t halo;
    int32_t lo_rank, hi_rank; /* neighbour ranks, -1 = none (end of the volume) */
} lsf_slab_layout;
typedef struct lsf_slab_part {
    lsf_grid grid;             /* z-range of this part */
    const int32_t *band_list[2]; /* NULL = dense walk */
    int64_t band_count[2];
    int32_t band_subset[2];
    int32_t n_lists;           /* 1 or 2 launches (INTERIOR + BOUNDARY band lists) */
    int32_t reserved;
} lsf_slab_part;
/* compact faces (optional): only the band voxels of the boundary slices travel -- every other voxel of a slab face
 * never changes.  [0] = lower side, [1] = upper side.  send_list: ascending local voxel indices of the band voxels in the
 * `halo` owned slices next to that neighbour; recv_list: the same for this rank's halo slices on that side (the
 * neighbour's send list, shifted: both ranks derive the lists from identical initial data, the caller verifies that the
 * counts agree before the first exchange); send_msg / recv_msg: device buffers of 4 * count floats. */
typedef struct lsf_slab_faces {
    const int32_t *send_list[2], *recv_list[2];
    float *send_msg[2], *recv_msg[2];
    int64_t send_count[2], recv_count[2];
} lsf_slab_faces;
/* helper of the compact-face plan: out[f] = the ascending merge of the ascending runs a[f] (n_a[f] entries) and b[f]
 * (n_b[f]), all entries distinct, for f < pairs <= 4, in ONE launch (a face's band voxels are the face slices' entries
 * of the INTERIOR and of the BOUNDARY list: both ranks must enumerate them in the same -- ascending -- order). */
int lsf_merge_sorted_runs(const int32_t *const *a, const int64_t *n_a, const int32_t *const *b, const int64_t *n_b,
                          int32_t *const *out, int32_t pairs, void *stream);
int lsf_slab_unique_id(const char *rccl_library_path, uint8_t *id_out128);
int lsf_slab_comm_create(const char *rccl_library_path, const uint8_t *id128, int32_t rank, int32_t world,
                         lsf_slab_comm **out);
int lsf_slab_comm_destroy(lsf_slab_comm *comm);
/* what RCCL itself says about the communicator: ncclCommUserRank and ncclCommCount (bench.py puts them on its N > 1 line) */
int lsf_slab_comm_info(lsf_slab_comm *comm, int32_t *rank_out, int32_t *nranks_out);
/* The cross-check of a call's compact faces ("the caller verifies that the counts agree"), without a host round trip in
 * front of the launches: _begin hands this rank's four counts (send lower, send upper, recv lower, recv upper) to an
 * ncclAllGather on the communicator's stream and returns at once; _end waits for it and copies every rank's four counts,
 * rank-major, into table[4 * world].  Every rank sees every row and so reaches the same verdict.  Every rank of the
 * communicator must call the pair at the same point of its call sequence (it is a collective). */
int lsf_slab_face_counts_begin(lsf_slab_comm *comm, const int64_t *counts4);
int lsf_slab_face_counts_end(lsf_slab_comm *comm, int64_t *table);
int lsf_slab_state_iteration(lsf_slab_comm *comm, const float *state_in, const float *canonical, float *state_out,
                             const lsf_slab_layout *layout, const lsf_slab_part *boundary_parts, int32_t n_boundary,
                             const lsf_slab_part *interior_parts, int32_t n_interior,
                             const lsf_slavcheva_params *params, const lsf_gate *gate, lsf_iteration_record *record,
                             int32_t exchange /* LSF_SLAB_* */,
                             const lsf_slab_faces *faces /* NULL: whole slices travel */, void *stream);

/* ---- a whole fixed-count call of a z-SLAB rank, enqueued by the library in two host calls (round 6) ---------------------
 * lsf_state_run_begin / _finish for one rank of a z-slab run: the loop of slavcheva_optimizer2d.py:354-388 over this
 * rank's slab, with the schedule the calls above implement one iteration at a time -- exchange groups of `halo`
 * iterations (iteration j of a group runs over the owned range widened by halo - 1 - j slices on every interior side;
 * the group's last iteration computes the boundary slices first, sends the faces on the communicator's stream while the
 * interior runs, and leaves the wait to the next iteration, LSF_SLAB_EXCHANGE_DEFERRED / LSF_SLAB_RESUME), compact faces
 * cross-checked with the neighbours (lsf_slab_face_counts_*; whole slices when a neighbour disagrees), the listed
 * finalize pass, and ONE gather of every rank's record words (ncclAllGather) so that all ranks decode the same records.
 * Caller shape: one rank of run_hierarchical_optimizer3d_multipair.py:403-432's loop, the volume cut along z.
 *   base: as lsf_state_run for the LOCAL array (owned slices + halos, grid.z_begin = 0, z_end = nz; z_global_offset as the
 *         slab's); slices must be a multiple of 1024 voxels (the cut positions are per-chunk prefix counts of the
 *         counting pass); box_scratch must be NULL; totals_device / totals_host hold 5 + 2 * LSF_SLAB_MAX_CUTS int64.
 *   lsf_slab_run_begin: launches the counting pass and the states' initialisation and RETURNS when the list sizes and the
 *         positions of the schedule's z cuts are on the host; it fills the out members: the caller allocates
 *         index_scratch (out_index_entries int32) and face_messages (4 * out_face_entries + 16 floats; NULL = whole faces).
 *   lsf_slab_run_finish: list fills, `iterations` iterations, lsf_state_finalize_listed into live_out (which holds the
 *         input live field), the record gather; RETURNS when both streams have drained, the records of ALL ranks decoded
 *         into `result` (energies summed over the ranks' owned slices, maxima over everything computed).  The caller
 *         checks the maxima: an update of one voxel or more inside an exchange group has read invalid halo slices
 *          -- every rank sees the same numbers and repeats the call on a wider slab.
 *         words_device: (1 + world) * iterations * LSF_RECORD_SLOTS * 4 int64; words_host (page-locked): world * ... . */
#define LSF_SLAB_MAX_CUTS 72
typedef struct lsf_slab_run {
    lsf_state_run base;
    lsf_slab_layout layout;
    int32_t exchange_interval;    /* iterations per exchange: layout.halo (exchange groups) or 1 */
    int32_t n_cuts;               /* out: the slices at which the band lists are cut, ascending ... */
    int32_t cut_slices[LSF_SLAB_MAX_CUTS];
    int64_t cut_entries[2][LSF_SLAB_MAX_CUTS]; /* out: ... and the number of INTERIOR / BOUNDARY entries in front of each */
    int64_t out_index_entries;    /* out: int32 elements of index_scratch lsf_slab_run_finish needs */
    int64_t out_face_entries;     /* out: band voxels of the four faces (send lower, send upper, recv lower, recv upper) */
} lsf_slab_run;
int lsf_slab_run_begin(lsf_slab_run *run, void *stream);
int lsf_slab_run_finish(const lsf_slab_run *run, lsf_slab_comm *comm, const lsf_slavcheva_params *params,
                        int32_t *list_interior, int32_t *list_boundary, int32_t *index_scratch, float *face_messages,
                        lsf_iteration_record *records, int32_t iterations, float *live_out, int64_t *words_device,
                        int64_t *words_host, lsf_state_run_result *result, void *stream);

/* the LAST pass of the zero-preserving filter at the voxels of a band list (axis = 2 in 3-D, 0 in 2-D:
 * math_utils/convolution.py:94-111,114-132; 3 / 5 / 7 / 9 taps) fused with lsf_slavcheva_update_rewarp
 * (slavcheva_optimizer2d.py:208-236): in_planar = the output of the passes before, zero_mask_source = the RAW gradient,
 * g_out_planar receives the final gradient; results are those of lsf_convolve_axis_listed + lsf_slavcheva_update_rewarp. */
int lsf_slavcheva_filter_update_rewarp(const float *in_planar, const float *zero_mask_source, const float *live,
                                       float *g_out_planar, float *warp_out_planar, float *live_out,
                                       const lsf_grid *grid, const lsf_slavcheva_params *params, int32_t axis,
                                       const double *taps_host, int32_t n_taps, const lsf_gate *gate,
                                       lsf_iteration_record *record, const int32_t *band_list, int64_t band_count,
                                       void *stream);

int lsf_slavcheva_update_rewarp(const float *live, const float *canonical, float *g_planar /* inout */,
                                float *warp_out_planar, float *live_out, const lsf_grid *grid,
                                const lsf_slavcheva_params *params, const lsf_gate *gate,
                                lsf_iteration_record *record, const int32_t *band_list /* may be NULL */,
                                int64_t band_count, void *stream);

/* ---- one energy term on its own: the term-level functions of nonrigid_opt/slavcheva/{data_term,smoothing_term,
 * level_set_term}.py, which the reference's tests, focus-point debugging and visualiser call one by one.  One launch
 * evaluates ONE term (below) at the selected voxels and writes any of: its gradient (float32), its per-voxel energy
 * contribution (float64, the float32 local value widened) and the sum of those contributions (float64, ADDED to
 * *energy_total by block reductions -- the caller zeroes it; the order of the additions varies between launches).
 *   term                           reference                                   reads
 *   LSF_TERM_DATA_BASIC            data_term.py:169-187, :334-349               live, canonical, live_gradient_x/y[/z]
 *   LSF_TERM_DATA_THRESHOLDED_FDM  data_term.py:190-227 (OOB neighbours read 1) the same
 *   LSF_TERM_TIKHONOV              smoothing_term.py:155-159 (-scipy laplace)   warp
 *   LSF_TERM_TIKHONOV_LOCAL        smoothing_term.py:103-139                    warp
 *   LSF_TERM_KILLING               smoothing_term.py:50-100                     warp
 *   LSF_TERM_LEVEL_SET             level_set_term.py:28-64                      live
 * live_gradient_* (caller's planes, data terms) are read only when gradient_out is given.
 * Energies: data terms 0.5*diff^2; Killing and level set their local form; the Tikhonov terms the per-location form of
 * smoothing_term.py:134-139 (energy_form LSF_TERM_ENERGY_LOCAL) or the np.gradient form of smoothing_term.py:162-177
 * (LSF_TERM_ENERGY_NP_GRADIENT; Tikhonov terms only).
 * selection: LSF_SELECT_ALL every voxel; LSF_SELECT_BAND every voxel, those outside the narrow-band union (|live| ==
 * |canonical| == 1, tsdf_set_routines.py:19-52) get gradient 0 and energy 0 (needs live and canonical);
 * LSF_SELECT_LIST the index_count flat voxel indices `indices` (device): outputs are then compact, entry k for indices[k]
 * (an index outside the array gets zeros).
 * Layout of warp and gradient_out: planar [c][voxel] (planes of nz*ny*nx entries, or index_count with a list), or
 * interleaved [voxel][c] with LSF_TERM_INTERLEAVED -- the reference's (..., D) arrays, no conversion launch.
 * LSF_TERM_COPY_IF_ZERO (TIKHONOV_LOCAL, KILLING): a neighbour outside the array or with norm 0 reads the centre value
 * (utils/sampling.py:91-96); without it a neighbour outside the array reads the centre (sampling.py:84-88).
 * LSF_TERM_IGNORE_IF_ZERO (TIKHONOV_LOCAL; KILLING accepts and ignores it, as the reference does): gradient and
 * energy 0 where a component of an existing 4-neighbour is 0.  Both flags have 2-D semantics only: LSF_ERR_BAD_ARGUMENT
 * in 3-D.  The grid must cover the whole array (z_begin 0, z_end nz). */
#define LSF_TERM_DATA_BASIC 0
#define LSF_TERM_DATA_THRESHOLDED_FDM 1
#define LSF_TERM_TIKHONOV 2
#define LSF_TERM_TIKHONOV_LOCAL 3
#define LSF_TERM_KILLING 4
#define LSF_TERM_LEVEL_SET 5
#define LSF_TERM_COPY_IF_ZERO 1
#define LSF_TERM_IGNORE_IF_ZERO 2
#define LSF_TERM_INTERLEAVED 4
#define LSF_SELECT_ALL 0
#define LSF_SELECT_BAND 1
#define LSF_SELECT_LIST 2
#define LSF_TERM_ENERGY_LOCAL 0
#define LSF_TERM_ENERGY_NP_GRADIENT 1

typedef struct lsf_term_params {
    double isomorphic_enforcement_factor_f64; /* Killing lambda as given: -2(1+lambda) is formed in double */
    float isomorphic_enforcement_factor;      /* float32(lambda) */
    float epsilon;                            /* level set, level_set_term.py:28 */
    float scaling_factor;                     /* data terms, data_term.py:182 / :335 */
    int32_t term;                             /* LSF_TERM_* */
    int32_t flags;                            /* LSF_TERM_COPY_IF_ZERO | LSF_TERM_IGNORE_IF_ZERO | LSF_TERM_INTERLEAVED */
    int32_t reserved;
} lsf_term_params;

/* replaces data_term.compute_data_term_gradient_vectorized / _direct / compute_data_term_energy_contribution /
 * compute_local_data_term* / data_term_at_location (data_term.py:169-237, 334-384), smoothing_term.compute_*
 * (smoothing_term.py:50-201) and level_set_term.level_set_term_at_location (level_set_term.py:28-64) */
int lsf_term_gradient(const float *live, const float *canonical, const float *live_gradient_x,
                      const float *live_gradient_y, const float *live_gradient_z, const float *warp,
                      float *gradient_out, double *energy_out, double *energy_total, const lsf_grid *grid,
                      const lsf_term_params *params, int32_t selection, int32_t energy_form, const int32_t *indices,
                      int64_t index_count, void *stream);

/* ---- a20: convergence statistics ---------------------------------------------------------------------
 * replaces cpp.build_warp_delta_statistics_2d / build_tsdf_difference_statistics_2d
 * (slavcheva_optimizer2d.py:394-398; known answer tests/test_slavcheva_optimizer.py:141-145).
 * out (device, 8 doubles each):
 *   warp:  [count_band, count_above_lo, max_len, sum_len, sum_len^2, argmax_linear_index, 0, scratch]
 *   tsdf:  [count, min, max, sum, sum^2, argmax_linear_index, 0, scratch]    of |canonical - live|   */
int lsf_warp_statistics(const float *warp_planar, const float *canonical, const float *live,
                        const lsf_grid *grid, float lower_threshold, double *out8, void *stream);
int lsf_tsdf_difference_statistics(const float *canonical, const float *live, const lsf_grid *grid,
                                   double *out8, void *stream);

/* ---- a21: TSDF from a depth image, nearest pixel (the input stage of the path) ------------------------
 * replaces tsdf/generation.py:130-207 (generate_2d_tsdf_field_from_depth_image_no_interpolation: grid dims 2,
 * field[y][x] with the field's y index as depth axis and y_voxel = 0, depth row image_y_coordinate) and
 * :356-437 (generate_3d_tsdf_field_from_depth_image: grid dims 3, field[z][y][x]); tsdf/common.py:34-47.
 * depth_image: DEVICE uint16 [image_height][image_width]. */
typedef struct lsf_tsdf_params {
    double intrinsics[4];        /* fx, fy, cx, cy */
    double depth_unit_ratio;     /* metres per depth unit */
    double voxel_size;           /* metres */
    double narrow_band_half_width; /* metres: narrow_band_width_voxels / 2 * voxel_size */
    float extrinsic[16];         /* camera_extrinsic_matrix, row-major 4x4, float32 */
    int32_t array_offset[3];     /* voxels (x, y, z) */
    int32_t image_width, image_height;
    int32_t image_y_coordinate;  /* 2-D only */
    float default_value;
    int32_t intrinsics_are_f32;  /* project in float32 (float32 intrinsic matrix) or float64 */
} lsf_tsdf_params;

int lsf_tsdf_generate_nearest(const uint16_t *depth_image, float *field, const lsf_grid *grid,
                              const lsf_tsdf_params *params, void *stream);

/* the two bilinear 2-D variants: replaces tsdf/generation.py:78-128 (generate_2d_tsdf_field_from_depth_image_bilinear_
 * image_space, method 1: blend the depth of the two pixels around the projection, one TSDF value) and :18-75
 * (…_bilinear_tsdf_space, method 2 = FilteringMethod.BILINEAR_VOXEL_SPACE: a TSDF value per pixel, then blend); grid
 * dims 2 only, out-of-image taps read 1 as in utils/sampling.py:35-55. */
int lsf_tsdf_generate_bilinear(const uint16_t *depth_image, float *field, const lsf_grid *grid,
                               const lsf_tsdf_params *params, int32_t method, void *stream);

/* EWA filters: replaces tsdf/ewa.py:230-353 (generate_tsdf_2d_ewa_image, method 3), :358-481 (…_ewa_tsdf, method 4),
 * :485-624 (…_ewa_tsdf_inclusive, method 5) for grid dims 2, and :59-184 (generate_tsdf_3d_ewa_image, method 3) for
 * grid dims 3 -- there field[a][b][c] has world x on array axis 0 and the depth axis on array axis 2 (the reference's
 * deliberate flip, tsdf/ewa.py:115-119).  params->intrinsics is ignored; the full matrix travels in ewa. */
typedef struct lsf_ewa_params {
    double covariance_camera_space[9]; /* R * (gaussian_covariance_scale*voxel_size*I) * R^T, row-major, float64 */
    double squared_radius_threshold;   /* 4 * gaussian_covariance_scale * voxel_size */
    float intrinsic_matrix[9];         /* row-major 3x3, float32 */
    int32_t method;                    /* 3 EWA_IMAGE_SPACE, 4 EWA_VOXEL_SPACE, 5 EWA_VOXEL_SPACE_INCLUSIVE */
} lsf_ewa_params;

int lsf_tsdf_generate_ewa(const uint16_t *depth_image, float *field, const lsf_grid *grid,
                          const lsf_tsdf_params *params, const lsf_ewa_params *ewa, void *stream);

/* nearest pixel on the inputs lsf_tsdf_generate_nearest refuses: the same reference functions (tsdf/generation.py:130-207,
 * :356-437), with the dtypes the reference's own arithmetic takes under numpy >= 2.
 * depth_image: DEVICE [image_height][image_width] of depth_dtype (LSF_DEPTH_*).  inf gives +1 like any depth beyond
 *   the band; d <= 0 leaves default_value.  float32 depth is scaled in float32 (depth * float32(depth_unit_ratio)),
 *   uint16 and float64 depth in float64.
 * array_offset: HOST, 3 doubles (x, y, z voxels, fractional allowed); params->array_offset is ignored.
 * extrinsic_f64: HOST, 16 doubles row-major: the product is evaluated in float64 and so is the projection.  NULL: the
 *   float32 params->extrinsic and the float32 product, as lsf_tsdf_generate_nearest.
 * The signed distance is taken in the promoted dtype of depth and camera-space point; a float32 distance is compared
 * with and divided by float32(narrow_band_half_width).  On uint16 depth, integral offsets and a float32 extrinsic the
 * result equals lsf_tsdf_generate_nearest's bit for bit; lsf_tsdf_params.array_offset is int32, so a fractional offset
 * needs this entry point. */
#define LSF_DEPTH_U16 0
#define LSF_DEPTH_F32 1
#define LSF_DEPTH_F64 2
int lsf_tsdf_generate_nearest_typed(const void *depth_image, int32_t depth_dtype, float *field, const lsf_grid *grid,
                                    const lsf_tsdf_params *params, const double *array_offset,
                                    const double *extrinsic_f64, void *stream);

/* ---- SDF-2-SDF rigid 2-D tracker ----------------------------------------------------------------------------------
 * replaces rigid_opt/sdf_gradient_field.py:13-38 (calculate_gradient_wrt_twist) and rigid_opt/sdf_2_sdf_optimizer2d.py:
 * 60-137 (Sdf2SdfOptimizer2d.optimize) on a square or rectangular 2-D field [height][width] (row = depth axis).
 * Per voxel, as the reference evaluates it:
 *   point      (x + offset_x) * voxel_size, (y + offset_z) * voxel_size in float64, rounded to float32
 *   twist^-1   twist_vector_to_matrix2d(-twist) (math_utils/transformation.py:11-23) -- not the true inverse
 *   trans      twist^-1 (float64) . point
 *   grad       np.gradient of the live field: central in the interior, one-sided at the edges (float32)
 *   g          ([grad_x, grad_y] . [[1, 0, trans_1], [0, 1, -trans_0]]) in float64, rounded to float32, then divided
 *              by float32(voxel_size)
 * The run (lsf_rigid_run) regenerates the live field every iteration from the live depth image under
 * twist_vector_to_matrix3d([t0, 0, t1, 0, t2, 0]) -- the float32-rounded twist, rotation about y by Rodrigues in float64
 * rounded to float32, float64 product (lsf_tsdf_generate_nearest_typed's arithmetic) -- then accumulates in float64
 *   A += g g^T (products float32), b += ((c - l) (float32) + g . twist) g, energy += (c [c > -eta] - l [l > -eta])^2
 * and updates twist += rate (A^-1 b - twist) (sdf_2_sdf_optimizer2d.py:92-126).  The update is skipped ("SINGULAR
 * MATRIX!", skipped = 1) when A holds a non-finite entry or its float64 LU with partial pivoting meets an exact zero
 * pivot: A == 0, a zero row and column (a twist-gradient component 0 at every voxel), any A found exactly singular --
 * where the reference's np.linalg.cond(A) is inf or NaN and it skips too.  A nearly singular A is inverted, as there. */
typedef struct lsf_rigid_params {
    lsf_tsdf_params tsdf;      /* intrinsics, ratio, voxel size, band, image extents and row, default value; its
                                  extrinsic and array_offset are ignored */
    double array_offset[3];    /* voxels (x, y, z), fractional allowed */
    double voxel_size;         /* calculate_gradient_wrt_twist's voxel_size (optimize()'s argument): the voxel points
                                  and the final division; tsdf.voxel_size is the generator's */
    double twist[3];           /* lsf_rigid_gradient: the twist (t_x, t_z, theta), float64 */
    double rate;               /* lsf_rigid_run: step of the update */
    float eta;                 /* lsf_rigid_run: float32(eta), weight threshold c > -eta */
    int32_t depth_dtype;       /* lsf_rigid_run: LSF_DEPTH_* of the live depth image */
    int32_t height, width;     /* field extents, >= 2 each */
    int32_t iterations;        /* lsf_rigid_run: >= 0 */
    int32_t reserved;
} lsf_rigid_params;

/* one record per iteration, LSF_RIGID_RECORD_DOUBLES doubles, written by the launch after it (lsf_rigid_run):
 *   [0, 3) twist* = A^-1 b (0 when skipped)   [3, 6) twist after the update   [6] energy   [7, 16) A row-major
 *   [16, 19) b   [19] skipped: 0 updated, 1 singular (not finite, or an exact zero pivot)   [20, 24) reserved */
#define LSF_RIGID_RECORD_DOUBLES 24
/* the launches of lsf_rigid_run use at most LSF_RIGID_MAX_BLOCKS workgroups; scratch holds two ping-pong buffers of
 * 10 float64 partial sums per workgroup (6 of A, 3 of b, energy) */
#define LSF_RIGID_MAX_BLOCKS 256
#define LSF_RIGID_SCRATCH_BYTES (2 * LSF_RIGID_MAX_BLOCKS * 10 * 8)

/* the gradient of live (DEVICE float32 [height][width]) with respect to params->twist: gradient_out DEVICE float32
 * [height][width][3].  One launch. */
int lsf_rigid_gradient(const float *live, float *gradient_out, const lsf_rigid_params *params, void *stream);

/* the whole optimize(): iterations launches of the fused iteration kernel, then one finishing launch, back to back on
 * stream with no host synchronisation.  canonical: DEVICE float32 [height][width]; live_depth: DEVICE depth image of
 * params->depth_dtype; twist_inout: DEVICE 3 doubles, read at the start, the final twist written by the finishing
 * launch; records: DEVICE iterations * LSF_RIGID_RECORD_DOUBLES doubles; scratch: DEVICE, LSF_RIGID_SCRATCH_BYTES. */
int lsf_rigid_run(const float *canonical, const void *live_depth, double *twist_inout, double *records,
                  void *scratch, const lsf_rigid_params *params, void *stream);

/* ---- SDF-2-SDF rigid 3-D tracker (6-DoF) ----------------------------------------------------------------------------
 * The reference has no 3-D tracker; this is its 2-D algorithm (rigid_opt/sdf_gradient_field.py:13-38,
 * rigid_opt/sdf_2_sdf_optimizer2d.py:60-137) lifted to a volume [depth][height][width] = [z][y][x], with the 2-D
 * kernel's dtypes.  The twist is (t_x, t_y, t_z, r_x, r_y, r_z) in twist_vector_to_matrix3d's layout
 * (math_utils/transformation.py:26-34); a 2-D twist (t0, t1, t2) is (t0, 0, t1, 0, t2, 0).  Per voxel:
 *   point      (index + offset) * voxel_size per axis in float64, rounded to float32
 *   p          twist_vector_to_matrix3d(-twist) (Rodrigues in float64) . (point, 1) in float64 -- the negated twist,
 *              not the inverse, as the 2-D reference's twist_vector_to_matrix2d(-twist)
 *   grad       np.gradient of the live volume: central inside, one-sided at all six faces (float32)
 *   g          [grad ; p x grad] in float64, rounded to float32, then divided by float32(voxel_size).  At r = 0 on a
 *              y-constant volume, (g_tx, g_tz, g_ry) is the 2-D g term for term; at r_y != 0 the 2-D matrix turns the
 *              x-z plane the other way from Rodrigues about y, and the two differ.
 * The run (lsf_rigid3d_run) regenerates the live volume every iteration under twist_vector_to_matrix3d of the
 * float32-rounded twist (Rodrigues in float64 rounded to float32, float64 product: lsf_tsdf_generate_nearest_typed's
 * arithmetic), then accumulates in float64
 *   A += g g^T (6 x 6, products float32), b += ((c - l) (float32) + g . twist) g, energy += (c [c > -eta] - l [l > -eta])^2
 * and updates twist += rate (A^-1 b - twist), the 2-D loop's step (sdf_2_sdf_optimizer2d.py:92-126).  The update is
 * skipped (skipped = 1) when A holds a non-finite entry or its float64 LU with partial pivoting meets an exact zero
 * pivot -- the 2-D rule; a wall facing the camera leaves the t_x, t_y and r_z columns zero.  A nearly singular A is
 * inverted. */
typedef struct lsf_rigid3d_params {
    lsf_tsdf_params tsdf;      /* intrinsics, ratio, voxel size, band, image extents, default value; its extrinsic,
                                  array_offset and image_y_coordinate are ignored */
    double array_offset[3];    /* voxels (x, y, z), fractional allowed */
    double voxel_size;         /* the gradient's voxel size (optimize()'s argument); tsdf.voxel_size is the generator's */
    double twist[6];           /* lsf_rigid3d_gradient: the twist, float64 */
    double rate;               /* lsf_rigid3d_run: step of the update */
    float eta;                 /* lsf_rigid3d_run: float32(eta), weight threshold c > -eta */
    int32_t depth_dtype;       /* LSF_DEPTH_* of the live depth image (the run; the gradient when live is NULL) */
    int32_t depth, height, width;  /* volume extents z, y, x, >= 2 each */
    int32_t iterations;        /* lsf_rigid3d_run: >= 0 */
} lsf_rigid3d_params;

/* one record per iteration, LSF_RIGID3D_RECORD_DOUBLES doubles, written by the launch after it (lsf_rigid3d_run);
 * each entry is the 6-DoF form of the 2-D record's (LSF_RIGID_RECORD_DOUBLES), which holds the values the reference's
 * loop prints or tests (sdf_2_sdf_optimizer2d.py:111 twist_star, :117 twist, :104-105 energy, :96-101 A and b, :110
 * the singular branch):
 *   [0, 6) twist* = A^-1 b (0 when skipped)   [6, 12) twist after the update   [12] energy   [13, 49) A row-major
 *   [49, 55) b   [55] skipped: 0 updated, 1 singular (not finite, or an exact zero pivot)   [56, 64) reserved */
#define LSF_RIGID3D_RECORD_DOUBLES 64
/* the launches of lsf_rigid3d_run use at most LSF_RIGID3D_MAX_BLOCKS workgroups; scratch holds two ping-pong buffers of
 * 28 float64 partial sums per workgroup (21 of A's upper triangle, 6 of b, energy) */
#define LSF_RIGID3D_MAX_BLOCKS 256
#define LSF_RIGID3D_SCRATCH_BYTES (2 * LSF_RIGID3D_MAX_BLOCKS * 28 * 8)

/* the gradient with respect to params->twist of a live volume, one launch.  live: DEVICE float32 [depth][height][width];
 * or NULL, and then the live volume is generated from live_depth (DEVICE depth image of params->depth_dtype) under
 * params->twist exactly as an iteration of lsf_rigid3d_run generates it.  live_out: NULL, or DEVICE float32
 * [depth][height][width] that receives the live volume used; gradient_out: NULL, or DEVICE float32
 * [depth][height][width][6].  At least one of the two outputs is given. */
int lsf_rigid3d_gradient(const float *live, const void *live_depth, float *live_out, float *gradient_out,
                         const lsf_rigid3d_params *params, void *stream);

/* the whole 6-DoF optimize(): iterations launches of the fused iteration kernel, then one finishing launch, back to back
 * on stream with no host synchronisation.  canonical: DEVICE float32 [depth][height][width]; live_depth: DEVICE depth
 * image of params->depth_dtype; twist_inout: DEVICE 6 doubles, read at the start, the final twist written by the
 * finishing launch; records: DEVICE iterations * LSF_RIGID3D_RECORD_DOUBLES doubles; scratch: DEVICE,
 * LSF_RIGID3D_SCRATCH_BYTES. */
int lsf_rigid3d_run(const float *canonical, const void *live_depth, double *twist_inout, double *records,
                    void *scratch, const lsf_rigid3d_params *params, void *stream);

/* ---- fusion of aligned frames into a canonical TSDF volume (KillingFusion / SobolevFusion's model update) -----------
 * The reference has no fusion code; the rule is this project's ("Fusion").  The model is two
 * float32 arrays of one shape, tsdf (starts at 1) and weight (starts at 0).  A voxel is observed when its live value l
 * satisfies -1 < l < 1 strictly (+-1 and NaN are not fused); there, in float32 with separately rounded operations,
 *   W1 = W + w,  tsdf = (W t + w l) / W1,  weight = min(W1, max_weight)
 * -- the average takes the uncapped W1.  A voxel that is not observed keeps its tsdf and weight bit for bit.
 * Each call writes a record of LSF_FUSION_RECORD_DOUBLES doubles: [0] fused (observed voxels), [1] first_seen (observed
 * voxels whose weight was 0), [2] sum over observed voxels of |t1 - t| (each term float32, summed in float64 in a fixed
 * order: reruns are bit-identical), [3] max |t1 - t|, [4..7] 0.  Voxels are taken four to a lane in flat order; the
 * per-workgroup partials (at most LSF_FUSION_MAX_BLOCKS) go to scratch and a finishing one-workgroup launch combines
 * them in a fixed order.  No host synchronisation. */
typedef struct lsf_fusion_params {
    lsf_tsdf_params tsdf;      /* depth mode: intrinsics, ratio, generator voxel size, band, image extents, default
                                  value; its extrinsic, array_offset and image_y_coordinate are ignored */
    double twist[6];           /* depth mode: the frame's twist (t_x, t_y, t_z, r_x, r_y, r_z), float64 */
    double array_offset[3];    /* depth mode: voxels (x, y, z), fractional allowed */
    int32_t depth, height, width; /* extents z, y, x, >= 1 each; volume mode fuses depth * height * width voxels */
    float weight;              /* w of the rule: finite, > 0 */
    float max_weight;          /* the cap: > 0, +inf allowed */
    int32_t depth_dtype;       /* depth mode: LSF_DEPTH_* of the depth image */
} lsf_fusion_params;
#define LSF_FUSION_RECORD_DOUBLES 8
#define LSF_FUSION_MAX_BLOCKS 2048
/* per-workgroup partials: fused, first_seen, sum, max */
#define LSF_FUSION_SCRATCH_BYTES (LSF_FUSION_MAX_BLOCKS * 4 * 8)

/* volume mode: fuse a given live field.  tsdf, weight: DEVICE float32, in/out, depth * height * width voxels each, two
 * distinct buffers; live: DEVICE float32 of the same count, aliasing neither (any contiguous shape: the index is flat);
 * record: DEVICE LSF_FUSION_RECORD_DOUBLES doubles; scratch: DEVICE, LSF_FUSION_SCRATCH_BYTES. */
int lsf_fusion_integrate_volume(float *tsdf, float *weight, const float *live, double *record, void *scratch,
                                const lsf_fusion_params *params, void *stream);

/* depth mode: the live value of every voxel of a [depth][height][width] volume generated from depth_image (DEVICE, of
 * params->depth_dtype) under params->twist exactly as lsf_rigid3d_gradient generates it (twist_vector_to_matrix3d of
 * the float32-rounded twist, nearest pixel), fused in the same pass; no live volume is written.  The result and the
 * record equal lsf_rigid3d_gradient's live_out followed by lsf_fusion_integrate_volume, bit for bit. */
int lsf_fusion_integrate_depth(float *tsdf, float *weight, const void *depth_image, double *record, void *scratch,
                               const lsf_fusion_params *params, void *stream);

/* ---- weighted depth-mode fusion with free-space carving ------------------------------------------------------------
 * The rule is INTEGRATION.md section 3, "Weighted fusion and carving".  Voxel, pixel (ix, iy), scaled depth and live
 * value l are lsf_fusion_integrate_depth's.  A voxel has a valid pixel when it lies in front of the camera, projects into
 * the image and the scaled depth there is > 0 or NaN; tsdf.default_value is not used.  With a valid pixel the voxel is in
 * band when -1 < l < 1 and, with carve != 0, carved when l == 1 exactly (the seen free space in front of the band), which
 * fuses l = 1.  Its weight is w_eff = weight * pixel_weight[iy][ix], one float32 multiply (weight itself without an
 * image); when w_eff is not finite and > 0 the voxel is left alone and counted.  Otherwise W1 = W + w_eff,
 * tsdf = (W t + w_eff l) / W1, weight = min(W1, max_weight) as above.  Every other voxel keeps its tsdf and weight bit
 * for bit.  The record: [0] fused (in-band updates), [1] first_seen (updates of either kind whose weight was 0), [2] sum
 * and [3] max of |t1 - t| over updates of either kind, [4] carved, [5] weight_rejected, [6..7] 0; summed as above, reruns
 * bit-identical.  With carve == 0 and no image, tsdf, weight and record [0..3] equal lsf_fusion_integrate_depth's bit for
 * bit whenever default_value is not strictly inside (-1, 1). */
typedef struct lsf_fusion_weighted_params {
    lsf_fusion_params fusion;  /* as lsf_fusion_integrate_depth reads it */
    int32_t carve;             /* 0: in-band voxels only; else also fuse +1 where l == 1 with a valid pixel */
    int32_t has_pixel_weight;  /* 0: pixel_weight is NULL; else it is given */
} lsf_fusion_weighted_params;
/* per-workgroup partials: fused, first_seen, sum, max, carved, weight_rejected */
#define LSF_FUSION_WEIGHTED_SCRATCH_BYTES (LSF_FUSION_MAX_BLOCKS * 6 * 8)

/* tsdf, weight, depth_image, record: as lsf_fusion_integrate_depth.  pixel_weight: NULL, or DEVICE float32
 * [image_height][image_width], overlapping neither tsdf nor weight; scratch: DEVICE,
 * LSF_FUSION_WEIGHTED_SCRATCH_BYTES.  Two launches, no host synchronisation. */
int lsf_fusion_integrate_depth_weighted(float *tsdf, float *weight, const void *depth_image, const float *pixel_weight,
                                        double *record, void *scratch, const lsf_fusion_weighted_params *params,
                                        void *stream);

/* ---- weighted depth-mode fusion that also fuses colour ---------------------------------------------------------------
 * The rule is INTEGRATION.md section 3, "Colour fusion".  Geometry is lsf_fusion_integrate_depth_weighted's with the same
 * weight, pixel_weight and carve: tsdf, weight and record [0..5] equal its results bit for bit.  The colour volume holds
 * one 16-byte record per voxel, float32 (R, G, B, Wc): the colour in units of the 8-bit image and the colour weight.  A
 * voxel is coloured when it has a valid pixel, its live value satisfies -colour_band < l < colour_band strictly and its
 * w_eff (the geometry rule's) is finite and > 0; with c_j = (float)colour_image[pixel][j], in float32 with separately
 * rounded operations,
 *   Wc1 = Wc + w_eff,  C_j = (Wc C_j + w_eff c_j) / Wc1,  Wc = min(Wc1, max_weight)
 * Carved voxels (l == 1) are never coloured, and every voxel that is not coloured keeps its 16 bytes bit for bit: colour
 * memory is read and written for coloured voxels only.  A rejected weight counts once, in record [5].  The record: [0..5]
 * as lsf_fusion_integrate_depth_weighted, [6] coloured, [7] first_coloured (coloured voxels whose Wc was 0), exact
 * counts; reruns bit-identical. */
typedef struct lsf_fusion_colour_params {
    lsf_fusion_weighted_params weighted; /* as lsf_fusion_integrate_depth_weighted reads it */
    float colour_band;                   /* finite, in (0, 1]: the coloured part of the band, in live-value units */
} lsf_fusion_colour_params;
/* per-workgroup partials: fused, first_seen, sum, max, carved, weight_rejected, coloured, first_coloured */
#define LSF_FUSION_COLOUR_SCRATCH_BYTES (LSF_FUSION_MAX_BLOCKS * 8 * 8)

/* tsdf, weight, depth_image, pixel_weight, record: as lsf_fusion_integrate_depth_weighted.  colour: DEVICE float32
 * [depth][height][width][4], in/out, 16-byte aligned.  colour_image: DEVICE uint8 [image_height][image_width][3] (R, G,
 * B), registered to the depth image.  scratch: DEVICE, LSF_FUSION_COLOUR_SCRATCH_BYTES.  tsdf, weight, colour,
 * colour_image, pixel_weight and depth_image must not overlap one another.  Two launches, no host synchronisation. */
int lsf_fusion_integrate_depth_colour(float *tsdf, float *weight, float *colour, const void *depth_image,
                                      const float *pixel_weight, const uint8_t *colour_image, double *record,
                                      void *scratch, const lsf_fusion_colour_params *params, void *stream);

/* ---- weighted depth-mode fusion through a non-rigid warp field -------------------------------------------------------
 * The rule is INTEGRATION.md section 3, "Warped depth fusion".  warp holds one displacement psi per voxel, float32
 * [depth][height][width][3] interleaved, channel 0 the x displacement, 1 y, 2 z, in voxels: the cumulative warp
 * HierarchicalOptimizer3d.optimize(canonical, live) returns, live(v + psi(v)) ~ canonical(v).  Voxel (x, y, z) observes
 * the frame at its warped point
 *   ((float)((((double)x + (double)psi_x) + array_offset[0]) * voxel_size), likewise y and z)
 * -- lsf_fusion_integrate_depth's voxel point with one float64 add in front, so psi = +-0 reproduces it exactly.  That
 * point is transformed, projected and compared with the depth at its pixel exactly as the voxel's centre is, and from
 * there on the rule is lsf_fusion_integrate_depth_weighted's (valid pixel, in band, carved at exactly +1 with carve,
 * w_eff = weight * pixel_weight[pixel], weight rejection) and, with a colour volume, lsf_fusion_integrate_depth_colour's
 * (colour band, the pixel's colour under w_eff).  A voxel whose psi has a component that is not finite is left alone,
 * its colour record too, and is counted in warp_rejected and in nothing else.  With psi = 0 everywhere tsdf, weight,
 * colour and record [0..7] equal those entry points' bit for bit.  The record has LSF_FUSION_WARPED_RECORD_DOUBLES
 * doubles: [0..7] as lsf_fusion_integrate_depth_colour ([6], [7] are 0 without colour), [8] warp_rejected; summed as
 * above, reruns bit-identical. */
typedef struct lsf_fusion_warped_params {
    lsf_fusion_colour_params colour; /* as lsf_fusion_integrate_depth_colour reads it; colour_band is checked with
                                        has_colour only */
    int32_t has_colour;              /* 0: colour and colour_image are NULL; else both are given */
} lsf_fusion_warped_params;
#define LSF_FUSION_WARPED_RECORD_DOUBLES 9
/* per-workgroup partials: the colour call's eight, warp_rejected */
#define LSF_FUSION_WARPED_SCRATCH_BYTES (LSF_FUSION_MAX_BLOCKS * 9 * 8)

/* tsdf, weight, depth_image, pixel_weight (NULL allowed): as lsf_fusion_integrate_depth_weighted.  colour, colour_image:
 * as lsf_fusion_integrate_depth_colour, both given or both NULL.  warp: DEVICE float32, 3 * depth * height * width, read
 * with 16-byte accesses when its base is 16-byte aligned.  record: DEVICE LSF_FUSION_WARPED_RECORD_DOUBLES doubles;
 * scratch: DEVICE, LSF_FUSION_WARPED_SCRATCH_BYTES.  tsdf, weight, colour, warp, depth_image, pixel_weight and
 * colour_image must not overlap one another.  Two launches, no host synchronisation. */
int lsf_fusion_integrate_depth_warped(float *tsdf, float *weight, float *colour, const float *warp,
                                      const void *depth_image, const float *pixel_weight, const uint8_t *colour_image,
                                      double *record, void *scratch, const lsf_fusion_warped_params *params,
                                      void *stream);

/* ---- a per-pixel confidence image for weighted fusion ----------------------------------------------------------------
 * c(u, v) = |n . r| min(1, (reference_depth / z)^2): the cosine between the pixel's unit ray r and its normal n, times
 * the inverse of the sensor's axial noise growth beyond reference_depth.  Every step is one float64 operation, in this
 * order, rounded once to float32 at the end ("Depth confidence"):
 *   x = (u - cx) / fx,  y = (v - cy) / fy,  len = sqrt((x x + y y) + 1),  dot = (n_x x + n_y y) + n_z,
 *   a = |dot| / len,  q = reference_depth / z,  s = q q,  m = s < 1 ? s : 1,  c = a m
 * c is 0 where z is not > 0 (NaN included) or where n is lsf_depth_pyramid's "no normal" value, all three components 0. */
typedef struct lsf_depth_confidence_params {
    double fx, fy, cx, cy;     /* intrinsics, pixels; finite, fx and fy non-zero */
    double reference_depth;    /* metres, finite and > 0 */
    int32_t height, width;     /* image extents, >= 1 each, at most 2^31 - 1 pixels */
} lsf_depth_confidence_params;

/* depth: DEVICE float32 [height][width], metres; normals: DEVICE float32 [height][width][3], camera coordinates (level 0
 * of lsf_depth_pyramid's outputs); confidence_out: DEVICE float32 [height][width], overlapping neither input.  One lane
 * per pixel, one launch, no host synchronisation. */
int lsf_depth_confidence(const float *depth, const float *normals, float *confidence_out,
                         const lsf_depth_confidence_params *params, void *stream);

/* ---- ray-casting the canonical TSDF into a depth (and normal) image -------------------------------------------------
 * The reference has no ray-caster; the arithmetic is this project's ("Ray-casting"), every
 * step one float64 operation.  The camera is the generator's: E = twist_vector_to_matrix3d of the float32-rounded
 * twist (lsf_fusion_integrate_depth's), world -> camera.  Pixel (u, v) casts the ray s ((u - cx) / fx, (v - cy) / fy, 1)
 * from the camera centre; voxel (i, j, k) of the [z][y][x] volume sits at ((k, j, i) + offset) * voxel_size.  The ray
 * is clipped to the box of valid sample positions and sampled at s = m * voxel_size / LSF_RAYCAST_STEPS_PER_VOXEL
 * (camera z, m >= 1 an integer).  A sample is trilinear in tsdf and valid only when all 8 corner weights are > 0.  The
 * surface is the first step whose previous sample is valid and > 0 and whose own sample is valid and <= 0; the depth is
 * refined linearly between the two.  One lane per pixel; a workgroup covers LSF_RAYCAST_TILE x LSF_RAYCAST_TILE pixels,
 * each wave an 8 x 8 block of them.  No host synchronisation. */
typedef struct lsf_raycast_params {
    double fx, fy, cx, cy;             /* intrinsics, pixels; finite, fx and fy non-zero */
    double depth_unit_ratio;           /* metres per unit of the fallback image (ignored without one) */
    double voxel_size;                 /* metres, finite and > 0 */
    double offset_x, offset_y, offset_z; /* array offset, voxels, fractional allowed */
    double t_x, t_y, t_z, r_x, r_y, r_z; /* the camera's twist, float64 (rounded to float32 as the generator does) */
    int32_t depth, height, width;      /* volume extents z, y, x, >= 2 each */
    int32_t image_height, image_width; /* output extents, >= 1 each, at most 2^31 - 1 pixels */
    int32_t fallback_dtype;            /* LSF_DEPTH_* of fallback_depth (ignored when it is NULL) */
} lsf_raycast_params;
#define LSF_RAYCAST_STEPS_PER_VOXEL 2
#define LSF_RAYCAST_TILE 16

/* tsdf, weight: DEVICE float32 [depth][height][width], two distinct buffers, read only.  depth_out: DEVICE float32
 * [image_height][image_width], camera z of the hit in metres, 0 where a ray hits nothing.  normals_out: NULL, or DEVICE
 * float32 [image_height][image_width][3], the unit normal in camera coordinates (central differences of trilinear
 * samples one voxel apart), 0 where there is no hit or a difference sample is invalid.  fallback_depth: NULL, or DEVICE
 * [image_height][image_width] of fallback_dtype; where a ray hits nothing its value times depth_unit_ratio is written
 * (float32 depth scaled in float32, uint16 and float64 in float64).  hit_count: NULL, or DEVICE one uint64 to which the
 * number of hit pixels is ADDED (exact).  No output may alias an input or another output. */
int lsf_raycast(const float *tsdf, const float *weight, const void *fallback_depth, float *depth_out, float *normals_out,
                uint64_t *hit_count, const lsf_raycast_params *params, void *stream);

/* lsf_raycast with the model's colour ("Ray-cast colour"): the same march, and depth_out,
 * normals_out, the fallback and hit_count equal lsf_raycast's bit for bit.  colour: DEVICE float32
 * [depth][height][width][4], the model's records (R, G, B in units of the 8-bit image, the colour weight), read only.
 * colour_out: DEVICE float32 [image_height][image_width][4].  A hit pixel takes the float64 voxel coordinates of its hit
 * point (the refined depth along the ray, before it is rounded) and samples R, G and B there trilinearly, each in float64
 * in the order of the tsdf sample; the sample is valid when the 8 corners lie inside the volume and all 8 colour weights
 * are > 0 (they are read first).  It stores (R, G, B, Y), Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 in float64, each
 * rounded to float32.  A pixel without a hit (one the fallback filled included) or without a valid sample gets four
 * NaNs.  colour and colour_out must not be NULL; no output may alias an input or another output. */
int lsf_raycast_colour(const float *tsdf, const float *weight, const float *colour, const void *fallback_depth,
                       float *depth_out, float *normals_out, float *colour_out, uint64_t *hit_count,
                       const lsf_raycast_params *params, void *stream);

/* ---- projective point-to-plane ICP against the ray-cast prediction -------------------------------------------------
 * The KinectFusion tracker; the reference has none, the arithmetic is this project's (INTEGRATION.md section 3,
 * "Projective ICP"), every step one float64 operation.  The prediction is lsf_raycast's depth and normals at twist_p
 * (camera E_p = twist_vector_to_matrix3d of the float32-rounded twist_p); a prediction pixel is usable when its depth is
 * > 0 and its normal non-zero.  The estimate is the float64 twist xi, its pose [Rodrigues(xi_r), xi_t] built from the
 * unrounded twist.  A live pixel (u, v) with depth d > 0 has the vertex v = d ((u - cx) / fx, (v - cy) / fy, 1), the
 * world point g = R^T (v - xi_t) and the prediction camera point q = R_p g + t_p; it associates with the prediction
 * pixel (rint(fx q_x / q_z + cx), rint(fy q_y / q_z + cy)) when q_z > 0, that pixel is in the image and usable, and
 * |g - V_w| <= max_distance, V_w the prediction vertex in world coordinates.  Residual r = N_w . (g - V_w), Jacobian
 * J = (N_w, g x N_w); each iteration sums A = sum J J^T, b = -sum J r, the energy sum r^2 and the correspondence count,
 * solves delta = A^-1 b (skipped as in the rigid trackers) and composes R' = R Rodrigues(delta_w)^T,
 * t' = xi_t - R' delta_t, xi' = (t', log R').  Levels run coarse first; a level of stride s uses the live pixels
 * (s i, s j) and associates into the full-resolution prediction.  One lane per strided live pixel, a wave per 8 x 8
 * block of them, a grid-stride loop over at most LSF_ICP_MAX_BLOCKS workgroups.  The partial sums cross launch
 * boundaries only: no float atomics, and a rerun is bit-identical. */
#define LSF_ICP_MAX_LEVELS 4
typedef struct lsf_icp_params {
    double fx, fy, cx, cy;             /* intrinsics, pixels; finite, fx and fy non-zero */
    double depth_unit_ratio;           /* metres per unit of the live depth image, finite */
    double max_distance;               /* metres, > 0 (inf allowed) */
    double twist_p[6];                 /* the prediction's twist, float64 (rounded to float32 as the ray-cast does) */
    int32_t height, width;             /* image extents of the live frame and the prediction, >= 1 each, at most
                                          2^31 - 1 pixels */
    int32_t depth_dtype;               /* LSF_DEPTH_* of the live depth image */
    int32_t levels;                    /* 1 .. LSF_ICP_MAX_LEVELS */
    int32_t iterations[LSF_ICP_MAX_LEVELS]; /* per level, coarse first, >= 0 */
    int32_t strides[LSF_ICP_MAX_LEVELS];    /* per level, >= 1 */
} lsf_icp_params;

/* one record per iteration, LSF_ICP_RECORD_DOUBLES doubles, written by the launch after it:
 *   [0, 6) delta = A^-1 b (0 when skipped)   [6, 12) twist after the update   [12] energy (sum r^2)   [13, 49) A
 *   row-major   [49, 55) b   [55] skipped: 0 updated, 1 singular (not finite, or an exact zero pivot)
 *   [56] correspondence count   [57] level   [58] pairs the normal-angle gate rejected (lsf_icp_run_pyramid; 0 from
 *   lsf_icp_run)   [59] photometric pair count   [60] photometric energy, sum r_I^2 (lsf_icp_run_photometric; 0 from
 *   the other two; lsf_icp_run_pyramid_photometric writes 58, 59 and 60)   [61] sum of the geometric weights w
 *   [62] sum of the photometric weights w_I   [63] geometric outliers (lsf_icp_run_robust and
 *   lsf_icp_run_pyramid_robust; 0 from the other four).  lsf_point_sdf_run writes the same record: [58] its pixels
 *   with a depth and no valid sample, [61] and [63] with a loss */
#define LSF_ICP_RECORD_DOUBLES 64
/* the launches of lsf_icp_run use at most LSF_ICP_MAX_BLOCKS workgroups; scratch holds two ping-pong buffers of 29
 * float64 partial sums per workgroup (21 of A's upper triangle, 6 of b, energy, count) */
#define LSF_ICP_MAX_BLOCKS 256
#define LSF_ICP_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 29 * 8)

/* the whole pyramid: sum(iterations) launches of the fused iteration kernel, then one finishing launch, back to back
 * on stream with no host synchronisation.  live_depth: DEVICE [height][width] of params->depth_dtype (float32 depth
 * scaled in float32, uint16 and float64 in float64); pred_depth: DEVICE float32 [height][width] in metres;
 * pred_normals: DEVICE float32 [height][width][3] in camera coordinates (lsf_raycast's outputs at twist_p);
 * twist_inout: DEVICE 6 doubles, read at the start, the final twist written by the finishing launch; records: DEVICE
 * sum(iterations) * LSF_ICP_RECORD_DOUBLES doubles; scratch: DEVICE, LSF_ICP_SCRATCH_BYTES; residuals_out: NULL, or
 * DEVICE float32 [height][width] that receives the last iteration's r, NaN where a pixel has no correspondence (or is
 * not on the last level's stride).  With sum(iterations) == 0 nothing is launched.  No output may alias an input or
 * another output. */
int lsf_icp_run(const void *live_depth, const float *pred_depth, const float *pred_normals, double *twist_inout,
                double *records, void *scratch, float *residuals_out, const lsf_icp_params *params, void *stream);

/* ---- the live depth pyramid: bilateral filter, depth-gated 2 x 2 means, per-level normals ---------------------------
 * The measurement stage KinectFusion puts in front of ICP; the reference has none.  The arithmetic is INTEGRATION.md
 * section 3 ("Depth pyramid"), every step one float64 operation.  Level 0 is the live depth scaled by depth_unit_ratio
 * (lsf_icp_run's scaling) and bilaterally filtered over the window |du|, |dv| <= radius (radius 0: unfiltered); level
 * l + 1 is the depth-gated mean of level l's 2 x 2 blocks; every level gets normals n = B x A of its forward
 * differences, 0 at the last row and column, at invalid depths and across a depth step > depth_gate.  Level l has
 * extents (height >> l, width >> l) and the intrinsics fx_l = fx_{l-1} / 2, fy_l = fy_{l-1} / 2,
 * cx_l = (cx_{l-1} - 0.5) / 2, cy_l = (cy_{l-1} - 0.5) / 2.  Levels are stored back to back, level 0 first. */
#define LSF_PYRAMID_MAX_RADIUS 8
typedef struct lsf_depth_pyramid_params {
    double fx, fy, cx, cy;     /* level-0 intrinsics, pixels; finite, fx and fy non-zero */
    double depth_unit_ratio;   /* metres per unit of the depth image, finite */
    double sigma_space;        /* pixels, finite and > 0 when radius > 0 */
    double sigma_range;        /* metres, finite and > 0 when radius > 0 */
    double depth_gate;         /* metres, > 0 (inf allowed) */
    int32_t height, width;     /* level-0 extents, >= 1 each, at most 2^31 - 1 pixels */
    int32_t depth_dtype;       /* LSF_DEPTH_* of the depth image */
    int32_t levels;            /* 1 .. LSF_ICP_MAX_LEVELS; height >> (levels - 1) and width >> (levels - 1) >= 1 */
    int32_t radius;            /* 0 .. LSF_PYRAMID_MAX_RADIUS */
} lsf_depth_pyramid_params;

/* depth_image: DEVICE [height][width] of depth_dtype.  pyramid_depth: DEVICE float32, sum over levels of
 * (height >> l) (width >> l) values, metres, 0 where invalid; pyramid_normals: DEVICE float32, three times that,
 * [y][x][3] per level, camera coordinates.  levels + 1 launches on stream with no host wait: the filter, one per
 * coarser level, one for the normals of every level.  No buffer may alias another. */
int lsf_depth_pyramid(const void *depth_image, float *pyramid_depth, float *pyramid_normals,
                      const lsf_depth_pyramid_params *params, void *stream);

/* ---- projective point-to-plane ICP over a depth pyramid, with a normal-angle gate ----------------------------------
 * lsf_icp_run's arithmetic, schedule and records, with the live pixels taken from a lsf_depth_pyramid output: the level
 * of iterations entry k (coarse first) is levels - 1 - k; every pixel of it is back-projected with that level's
 * intrinsics and associated into the full-resolution prediction with the level-0 ones.  With angle_gate != 0 a pair is
 * kept only when the live normal n is non-zero and (R^T n) . N_w >= cos_max_angle, tested after the distance; record
 * slot 58 counts the pairs the gate rejects.  The partial sums hold a 30th entry (that count), hence the scratch
 * size. */
typedef struct lsf_icp_pyramid_params {
    double fx, fy, cx, cy;             /* level-0 intrinsics, pixels; finite, fx and fy non-zero */
    double max_distance;               /* metres, > 0 (inf allowed) */
    double cos_max_angle;              /* the gate: -1 .. 1 */
    double twist_p[6];                 /* the prediction's twist, float64 (rounded to float32 as the ray-cast does) */
    int32_t height, width;             /* level-0 extents of the live pyramid and the prediction */
    int32_t pyramid_levels;            /* levels the live pyramid holds, 1 .. LSF_ICP_MAX_LEVELS */
    int32_t levels;                    /* levels tracked, 1 .. pyramid_levels */
    int32_t angle_gate;                /* 0: no gate, else gate at cos_max_angle */
    int32_t iterations[LSF_ICP_MAX_LEVELS]; /* per tracked level, coarse first, >= 0 */
} lsf_icp_pyramid_params;
#define LSF_ICP_PYRAMID_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 30 * 8)

/* live_depth, live_normals: lsf_depth_pyramid's outputs for (height, width, pyramid_levels); pred_depth,
 * pred_normals, twist_inout, records: as lsf_icp_run; scratch: DEVICE, LSF_ICP_PYRAMID_SCRATCH_BYTES; residuals_out:
 * NULL, or DEVICE float32 of the last iteration's level extents, r there, NaN where a pixel has no correspondence.
 * sum(iterations) + 1 launches, none when sum(iterations) == 0.  No output may alias an input or another output. */
int lsf_icp_run_pyramid(const float *live_depth, const float *live_normals, const float *pred_depth,
                        const float *pred_normals, double *twist_inout, double *records, void *scratch,
                        float *residuals_out, const lsf_icp_pyramid_params *params, void *stream);

/* ---- joint geometric and photometric ICP on the strided path -------------------------------------------------------
 * lsf_icp_run's pairs, schedule and records, and for every live pixel with a geometric pair an intensity term against
 * the ray-cast colour image (lsf_raycast_colour at twist_p; INTEGRATION.md section 3, "Photometric ICP"), every step
 * one float64 operation.  With q the pixel's point in the prediction's camera: pu = (fx q_x) / q_z + cx,
 * pv = (fy q_y) / q_z + cy (the values before rint), x0 = floor(pu), y0 = floor(pv); the term needs 0 <= x0,
 * x0 + 1 <= width - 1, 0 <= y0, y0 + 1 <= height - 1 and the four Y = pred_colour[..][3] at (x0, y0), (x0 + 1, y0),
 * (x0, y0 + 1), (x0 + 1, y0 + 1) finite.  I_p is their bilinear interpolant at (pu, pv), (I_u, I_v) its exact
 * derivatives, I_l = ((0.299 R + 0.587 G) + 0.114 B) / 255 of the live pixel's bytes, r_I = I_p - I_l, kept when
 * |r_I| <= max_intensity_difference.  c = (I_u fx / q_z, I_v fy / q_z, -((I_u fx) q_x + (I_v fy) q_y) / (q_z q_z)),
 * a = R_p^T c, J_I = (a, g x a).  lambda J_I and lambda r_I go into the same A and b as the geometric term.  Record
 * slot 59 is the photometric pair count, slot 60 sum r_I^2 (unscaled); slot 12 stays the geometric energy, slot 56 the
 * geometric count, slot 58 is 0. */
typedef struct lsf_icp_photometric_params {
    double fx, fy, cx, cy;             /* as lsf_icp_params */
    double depth_unit_ratio;
    double max_distance;
    double photometric_weight;         /* lambda: finite and > 0 */
    double max_intensity_difference;   /* the gate on |r_I|, units of Y (0 .. 1): > 0 (inf allowed) */
    double twist_p[6];
    int32_t height, width;
    int32_t depth_dtype;
    int32_t levels;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    int32_t strides[LSF_ICP_MAX_LEVELS];
} lsf_icp_photometric_params;
/* 31 partial sums per workgroup: lsf_icp_run's 29, the photometric pair count, sum r_I^2 */
#define LSF_ICP_PHOTOMETRIC_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 31 * 8)

/* live_depth, pred_depth, pred_normals, twist_inout, records, residuals_out: as lsf_icp_run.  live_colour: DEVICE uint8
 * [height][width][3], registered to the depth; pred_colour: DEVICE float32 [height][width][4], lsf_raycast_colour's
 * output at twist_p; scratch: DEVICE, LSF_ICP_PHOTOMETRIC_SCRATCH_BYTES; intensity_residuals_out: NULL, or DEVICE
 * float32 [height][width] that receives the last iteration's r_I, NaN where a pixel has no photometric term (or is not
 * on the last level's stride).  sum(iterations) + 1 launches, none when sum(iterations) == 0; no float atomics, no host
 * wait, a rerun is bit-identical.  No output may alias an input or another output. */
int lsf_icp_run_photometric(const void *live_depth, const uint8_t *live_colour, const float *pred_depth,
                            const float *pred_normals, const float *pred_colour, double *twist_inout, double *records,
                            void *scratch, float *residuals_out, float *intensity_residuals_out,
                            const lsf_icp_photometric_params *params, void *stream);

/* ---- the intensity pyramids of photometric ICP over the depth pyramid ------------------------------------------------
 * Extends lsf_depth_pyramid's layout to intensities ("Intensity pyramid"), every step one
 * float64 operation.  Level 0 of a LSF_INTENSITY_SOURCE_COLOUR pyramid is float32(((0.299 R + 0.587 G) + 0.114 B) /
 * 255) of the image's bytes, lsf_icp_run_photometric's I_l; level 0 of a LSF_INTENSITY_SOURCE_PREDICTION pyramid is the
 * fourth channel (Y) of lsf_raycast_colour's image, copied bit for bit, NaNs included.  Level l + 1 has extents
 * (height >> (l + 1), width >> (l + 1)); with the 2 x 2 block q00, q10 (one row) and q01, q11 (the next) of level l
 * its value is float32(((q00 + q10) + (q01 + q11)) / 4), and NaN when one of the four is not finite.  Levels are stored
 * back to back, level 0 first. */
#define LSF_INTENSITY_SOURCE_COLOUR 0     /* image: DEVICE uint8 [height][width][3] */
#define LSF_INTENSITY_SOURCE_PREDICTION 1 /* image: DEVICE float32 [height][width][4], Y last */
typedef struct lsf_intensity_pyramid_params {
    int32_t height, width;     /* level-0 extents, >= 1 each, at most 2^31 - 1 pixels */
    int32_t levels;            /* 1 .. LSF_ICP_MAX_LEVELS; height >> (levels - 1) and width >> (levels - 1) >= 1 */
    int32_t source;            /* LSF_INTENSITY_SOURCE_* */
} lsf_intensity_pyramid_params;

/* image: as params->source says.  pyramid_intensity: DEVICE float32, sum over levels of (height >> l) (width >> l)
 * values, overlapping image nowhere.  `levels` launches on stream, one lane per output pixel, with no host wait and
 * no atomics. */
int lsf_intensity_pyramid(const void *image, float *pyramid_intensity, const lsf_intensity_pyramid_params *params,
                          void *stream);

/* ---- joint geometric and photometric ICP over the depth pyramid ------------------------------------------------------
 * Extends lsf_icp_run_pyramid by lsf_icp_run_photometric's term ("Photometric ICP").  The
 * geometric pair of a pixel of pyramid level L is lsf_icp_run_pyramid's exactly, gate included, against the
 * full-resolution prediction.  A pixel with a pair gets the intensity term at its own level: with the level's
 * intrinsics fx_L, fy_L, cx_L, cy_L and extents (w_L, h_L) = (width >> L, height >> L), pu = (fx_L q_x) / q_z + cx_L,
 * pv = (fy_L q_y) / q_z + cy_L, x0 = floor(pu), y0 = floor(pv); the term needs 0 <= x0, x0 + 1 <= w_L - 1, 0 <= y0,
 * y0 + 1 <= h_L - 1 and the four values of level L of pred_intensity at (x0, y0) .. (x0 + 1, y0 + 1) finite.  I_p, I_u
 * and I_v are lsf_icp_run_photometric's, I_l is level L of live_intensity at the live pixel, r_I = I_p - I_l is kept
 * when |r_I| <= max_intensity_difference, and the Jacobian is lsf_icp_run_photometric's with fx_L, fy_L.  32 partial
 * sums per workgroup: lsf_icp_run's 29, the gate's rejections (record slot 58), the photometric pair count (59) and
 * sum r_I^2 (60). */
typedef struct lsf_icp_pyramid_photometric_params {
    double fx, fy, cx, cy;             /* as lsf_icp_pyramid_params */
    double max_distance;
    double cos_max_angle;
    double photometric_weight;         /* lambda: finite and > 0 */
    double max_intensity_difference;   /* the gate on |r_I|, units of Y (0 .. 1): > 0 (inf allowed) */
    double twist_p[6];
    int32_t height, width;
    int32_t pyramid_levels;            /* levels the three live and prediction pyramids hold */
    int32_t levels;
    int32_t angle_gate;
    int32_t reserved;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
} lsf_icp_pyramid_photometric_params;
#define LSF_ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 32 * 8)

/* live_depth, live_normals, pred_depth, pred_normals, twist_inout, records, residuals_out: as lsf_icp_run_pyramid.
 * live_intensity, pred_intensity: lsf_intensity_pyramid's outputs for (height, width, pyramid_levels), of the frame's
 * colour image and of lsf_raycast_colour's image at twist_p; scratch: DEVICE,
 * LSF_ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES; intensity_residuals_out: NULL, or DEVICE float32 of the last iteration's
 * level extents, r_I there, NaN where a pixel has no photometric term.  sum(iterations) + 1 launches, none when
 * sum(iterations) == 0; no float atomics, no host wait, a rerun is bit-identical.  No output may alias an input or
 * another output. */
int lsf_icp_run_pyramid_photometric(const float *live_depth, const float *live_normals, const float *live_intensity,
                                    const float *pred_depth, const float *pred_normals, const float *pred_intensity,
                                    double *twist_inout, double *records, void *scratch, float *residuals_out,
                                    float *intensity_residuals_out,
                                    const lsf_icp_pyramid_photometric_params *params, void *stream);

/* ---- robust ICP: Huber and Tukey weights on both terms, strided and pyramid ------------------------------------------
 * An iteratively reweighted solve ("Robust ICP"): the pairs, gates, schedule and records of
 * lsf_icp_run_photometric (lsf_icp_run's without the images), with every pair's rows of the normal equations scaled by
 * a weight of its own residual at the current twist, every step one float64 operation.  With a = |r| and the scale s:
 *   LSF_ICP_LOSS_HUBER  w = (a <= s) ? 1 : s / a               outlier: a > s
 *   LSF_ICP_LOSS_TUKEY  t = r / s, u = 1 - t t, w = (a < s) ? u u : 0   outlier: a >= s
 * A geometric pair (J, r) adds wJ_i = w J_i, A_ij += wJ_i J_j, b_i -= wJ_i r and (w r) r to the energy.  A photometric
 * term takes w_I from the unscaled r_I and intensity_scale, applies it to lambda J_I and lambda r_I in the same way and
 * adds (w_I r_I) r_I to the photometric energy.  The distance gate, the normal-angle gate and max_intensity_difference
 * stay hard gates in front of the weight; a pair with w = 0 still counts; the residual images keep the unweighted r and
 * r_I.  An infinite scale makes every weight exactly 1 and every product above exact, so a call with both scales
 * infinite equals the plain entry point's twist, residuals and record slots 0 .. 60 bit for bit.  Record slot 61 is
 * sum w over the geometric pairs, 62 sum w_I over the photometric pairs, 63 the geometric outliers.  No default scale
 * is right across sensors: the caller chooses both. */
#define LSF_ICP_LOSS_HUBER 1
#define LSF_ICP_LOSS_TUKEY 2
typedef struct lsf_icp_robust_params {
    double fx, fy, cx, cy;             /* as lsf_icp_photometric_params, member for member */
    double depth_unit_ratio;
    double max_distance;
    double photometric_weight;         /* lambda: finite and > 0 with the colour images, 0 without them */
    double max_intensity_difference;   /* with the colour images: > 0 (inf allowed); not read without them */
    double twist_p[6];
    int32_t height, width;
    int32_t depth_dtype;
    int32_t levels;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    int32_t strides[LSF_ICP_MAX_LEVELS];
    int32_t loss;                      /* LSF_ICP_LOSS_* */
    double scale;                      /* of r, metres: > 0 (inf allowed: least squares) */
    double intensity_scale;            /* of r_I, units of Y (0 .. 1): > 0 (inf allowed: least squares) */
} lsf_icp_robust_params;
/* at most 34 partial sums per workgroup: lsf_icp_run_photometric's 31, sum w, sum w_I, the outliers */
#define LSF_ICP_ROBUST_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 34 * 8)

/* lsf_icp_run_photometric's arguments, and weights_out: NULL, or DEVICE float32 [height][width] that receives the last
 * iteration's geometric w, laid out like residuals_out (NaN where a pixel has no correspondence or is not on the last
 * level's stride), written by the launch that writes the residuals.  live_colour and pred_colour are optional: with
 * both NULL, photometric_weight == 0 and intensity_residuals_out NULL the call is the geometric solve of lsf_icp_run
 * with weights.  One of the two NULL without the other, a non-zero photometric_weight without them, an unknown loss, a
 * scale or intensity_scale that is NaN or <= 0 return LSF_ERR_BAD_ARGUMENT.  scratch: DEVICE,
 * LSF_ICP_ROBUST_SCRATCH_BYTES.  sum(iterations) + 1 launches, none when sum(iterations) == 0; no float atomics, no host
 * wait, a rerun is bit-identical.  No output (weights_out included) may alias an input or another output. */
int lsf_icp_run_robust(const void *live_depth, const uint8_t *live_colour, const float *pred_depth,
                       const float *pred_normals, const float *pred_colour, double *twist_inout, double *records,
                       void *scratch, float *residuals_out, float *intensity_residuals_out, float *weights_out,
                       const lsf_icp_robust_params *params, void *stream);

typedef struct lsf_icp_pyramid_robust_params {
    double fx, fy, cx, cy;             /* as lsf_icp_pyramid_photometric_params, member for member */
    double max_distance;
    double cos_max_angle;
    double photometric_weight;         /* lambda: finite and > 0 with the intensity pyramids, 0 without them */
    double max_intensity_difference;   /* with the intensity pyramids: > 0 (inf allowed); not read without them */
    double twist_p[6];
    int32_t height, width;
    int32_t pyramid_levels;
    int32_t levels;
    int32_t angle_gate;
    int32_t reserved;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    int32_t loss;                      /* LSF_ICP_LOSS_* */
    double scale;                      /* of r, metres: > 0 (inf allowed: least squares) */
    double intensity_scale;            /* of r_I, units of Y (0 .. 1): > 0 (inf allowed: least squares) */
} lsf_icp_pyramid_robust_params;
/* at most 35 partial sums per workgroup: lsf_icp_run_pyramid_photometric's 32, sum w, sum w_I, the outliers */
#define LSF_ICP_PYRAMID_ROBUST_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 35 * 8)

/* lsf_icp_run_pyramid_photometric's arguments, and weights_out: NULL, or DEVICE float32 of the last iteration's level
 * extents, the geometric w there, NaN where a pixel has no correspondence.  live_intensity and pred_intensity are
 * optional under lsf_icp_run_robust's rules: with both NULL, photometric_weight == 0 and intensity_residuals_out NULL
 * the call is lsf_icp_run_pyramid with weights.  The refusals are lsf_icp_run_pyramid's and lsf_icp_run_robust's.
 * scratch: DEVICE, LSF_ICP_PYRAMID_ROBUST_SCRATCH_BYTES.  sum(iterations) + 1 launches, none when sum(iterations) == 0;
 * no float atomics, no host wait, a rerun is bit-identical.  No output (weights_out included) may alias an input or
 * another output. */
int lsf_icp_run_pyramid_robust(const float *live_depth, const float *live_normals, const float *live_intensity,
                               const float *pred_depth, const float *pred_normals, const float *pred_intensity,
                               double *twist_inout, double *records, void *scratch, float *residuals_out,
                               float *intensity_residuals_out, float *weights_out,
                               const lsf_icp_pyramid_robust_params *params, void *stream);

/* ---- point-to-SDF tracking: the live points against the canonical TSDF itself ------------------------------------------
 * The tracker of Bylow et al. (RSS 2013); the reference has none, the arithmetic is this project's (INTEGRATION.md
 * section 3, "Point-to-SDF tracking"), every step one float64 operation.  The estimate, the live vertex v, the world
 * point g = R^T (v - xi_t), the strided levels, the schedule, the solve and the composed update are lsf_icp_run's.
 * There is no prediction: g is taken to voxel coordinates p_j = g_j / voxel_size - offset_j (lsf_raycast's convention)
 * and the model is sampled there exactly as lsf_raycast samples it -- valid only for p_j in [0, n_j - 1) on every axis
 * and all 8 corner weights > 0 (read first), phi lerped x, then y, then z.  The same 8 corners t0 .. t7 (x fastest)
 * give the gradient in voxel units,
 *   d_x = ((t1 - t0) hy + (t3 - t2) fy) hz + ((t5 - t4) hy + (t7 - t6) fy) fz
 *   d_y = (c01 - c00) hz + (c11 - c10) fz        d_z = c1 - c0
 * with the sample's f, h = 1 - f and its intermediate lerps c00 .. c11, c0, c1.  With mu = narrow_band_width_voxels *
 * voxel_size: r = mu phi, grad_j = (mu d_j) / voxel_size.  A pixel is a pair when its depth is > 0, the sample is
 * valid, |r| <= max_distance and grad != 0; J = (grad, g x grad), A += J J^T, b -= J r, energy += r^2.  With a loss
 * (LSF_ICP_LOSS_HUBER / _TUKEY) a pair's rows are scaled by w(r) as in lsf_icp_run_robust; an infinite scale gives
 * the loss-free call bit for bit.  Records: lsf_icp_run's LSF_ICP_RECORD_DOUBLES and slots; [58] counts the pixels that
 * had a depth but no valid sample, [61] and [63] are sum w and the outliers with a loss, every other slot past 57 is
 * 0.  One lane per strided live pixel, a wave per 8 x 8 block of them (its 16 gathers per pixel share cache lines), a
 * grid-stride loop over at most LSF_ICP_MAX_BLOCKS workgroups. */
#define LSF_POINT_SDF_LOSS_NONE 0
typedef struct lsf_point_sdf_params {
    double fx, fy, cx, cy;             /* intrinsics, pixels; finite, fx and fy non-zero */
    double depth_unit_ratio;           /* metres per unit of the live depth image, finite */
    double max_distance;               /* metres, > 0 (inf allowed): the gate on |r| */
    double voxel_size;                 /* metres, finite and > 0 */
    double offset_x, offset_y, offset_z; /* array offset, voxels, finite, fractional allowed */
    double narrow_band_width_voxels;   /* the truncation distance in voxels, finite and > 0 */
    double scale;                      /* of r, metres, > 0 (inf allowed); not read without a loss */
    int32_t depth, height, width;      /* volume extents z, y, x, >= 2 each */
    int32_t image_height, image_width; /* live image extents, >= 1 each, at most 2^31 - 1 pixels */
    int32_t depth_dtype;               /* LSF_DEPTH_* of the live depth image */
    int32_t levels;                    /* 1 .. LSF_ICP_MAX_LEVELS */
    int32_t iterations[LSF_ICP_MAX_LEVELS]; /* per level, coarse first, >= 0 */
    int32_t strides[LSF_ICP_MAX_LEVELS];    /* per level, >= 1 */
    int32_t loss;                      /* LSF_POINT_SDF_LOSS_NONE, LSF_ICP_LOSS_HUBER or LSF_ICP_LOSS_TUKEY */
} lsf_point_sdf_params;
/* at most 33 partial sums per workgroup: lsf_icp_run's 29, the pixels without a valid sample, sum w, (sum w_I, not
 * used,) the outliers */
#define LSF_POINT_SDF_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 33 * 8)

/* tsdf, weight: DEVICE float32 [depth][height][width], two distinct buffers, read only.  live_depth, twist_inout,
 * records: as lsf_icp_run; scratch: DEVICE, LSF_POINT_SDF_SCRATCH_BYTES; residuals_out: NULL, or DEVICE float32
 * [image_height][image_width] that receives the last iteration's r, NaN where a pixel has no pair (or is not on the
 * last level's stride); weights_out: NULL, or (with a loss only) DEVICE float32 of the same extents, w where
 * residuals_out has r.  sum(iterations) + 1 launches back to back, none when sum(iterations) == 0; no float atomics,
 * no host wait, a rerun is bit-identical.  No output may alias an input or another output. */
int lsf_point_sdf_run(const float *tsdf, const float *weight, const void *live_depth, double *twist_inout,
                      double *records, void *scratch, float *residuals_out, float *weights_out,
                      const lsf_point_sdf_params *params, void *stream);

/* ---- point-to-SDF tracking with a colour term against the colour volume, strided and on the depth pyramid --------------
 * INTEGRATION.md section 3 ("Point-to-SDF tracking", "The colour term" and "The pyramid source").  The geometric pair is
 * lsf_point_sdf_run's, unchanged.  A pixel with a geometric pair also gets a colour term at the same voxel coordinates
 * p, hence the same cell and fractions f, h: the 8 corner records (R, G, B, W) of the colour volume (x fastest, then y,
 * then z; one 16-byte load each) must all have W > 0; y_k = ((0.299 R_k + 0.587 G_k) + 0.114 B_k) / 255 in float64;
 * Y and dY are the formulas of phi and d above on the corner values y_k.  r_I = Y - I_l, kept when
 * |r_I| <= max_intensity_difference (NaN fails), with I_l the live pixel's own intensity: on the strided source
 * ((0.299 R + 0.587 G) + 0.114 B) / 255 of its three bytes, unrounded, on the pyramid the pixel of its level of
 * lsf_intensity_pyramid's output.  gI_j = dY_j / voxel_size, J_I = (gI, g x gI); lambda = photometric_weight scales
 * first, J^ = lambda J_I, r^ = lambda r_I, then A += J^ J^^T, b -= J^ r^ into the same 27 sums.  Record slots 59 and 60
 * are the photometric pairs and the unscaled sum r_I^2.  With a loss w_I comes from the unscaled r_I and
 * intensity_scale, scales J^ and r^ as in lsf_icp_run_robust, (w_I r_I) r_I goes to slot 60 and sum w_I to slot 62; an
 * infinite scale gives the loss-free run bit for bit.
 * The pyramid source: entry k of iterations runs on level levels - 1 - k of lsf_depth_pyramid's depth output, every
 * pixel (u, v) of it, float32 metres valid when > 0, back-projected with that level's intrinsics; from the vertex on
 * the body is the strided one.  There is no normal-angle gate and the pyramid's normals are not read.  Record slot 57
 * is the entry index, slot 58 still the pixels with a depth and no valid sample. */
typedef struct lsf_point_sdf_photometric_params {
    double fx, fy, cx, cy;             /* lsf_point_sdf_params, member for member */
    double depth_unit_ratio;
    double max_distance;
    double voxel_size;
    double offset_x, offset_y, offset_z;
    double narrow_band_width_voxels;
    double scale;
    int32_t depth, height, width;
    int32_t image_height, image_width;
    int32_t depth_dtype;
    int32_t levels;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    int32_t strides[LSF_ICP_MAX_LEVELS];
    int32_t loss;
    double photometric_weight;         /* lambda: finite and > 0 with the colour inputs, 0 without them */
    double max_intensity_difference;   /* the gate on |r_I|, units of Y (0 .. 1): > 0 (inf allowed) */
    double intensity_scale;            /* of r_I, units of Y, > 0 (inf allowed); not read without a loss */
} lsf_point_sdf_photometric_params;
/* at most 35 partial sums per workgroup: lsf_point_sdf_run's 30, the photometric pairs, sum r_I^2, sum w, sum w_I,
 * the outliers */
#define LSF_POINT_SDF_COLOUR_SCRATCH_BYTES (2 * LSF_ICP_MAX_BLOCKS * 35 * 8)

/* lsf_point_sdf_run's arguments, and colour: NULL, or the model's DEVICE float32 [depth][height][width][4] colour
 * volume (lsf_fusion's (R, G, B, W) records), 16-byte aligned; live_colour: NULL, or the frame's DEVICE uint8
 * [image_height][image_width][3]; both or neither: with both NULL, photometric_weight == 0 and
 * intensity_residuals_out NULL the call is lsf_point_sdf_run.  intensity_residuals_out: NULL, or DEVICE float32
 * [image_height][image_width] that receives the last iteration's r_I, NaN where a pixel has no colour term.  scratch:
 * DEVICE, LSF_POINT_SDF_COLOUR_SCRATCH_BYTES.  Refused (LSF_ERR_BAD_ARGUMENT, before any launch): what
 * lsf_point_sdf_run refuses, one colour input without the other, a non-zero photometric_weight without both or a zero
 * one with them, a photometric_weight that is negative or not finite, a max_intensity_difference that is NaN or <= 0,
 * an intensity_scale that is NaN or <= 0 with a loss, a colour volume off 16-byte alignment.  sum(iterations) + 1
 * launches, none when sum(iterations) == 0; no float atomics, no host wait, a rerun is bit-identical.  No output may
 * alias an input or another output. */
int lsf_point_sdf_run_photometric(const float *tsdf, const float *weight, const float *colour, const void *live_depth,
                                  const uint8_t *live_colour, double *twist_inout, double *records, void *scratch,
                                  float *residuals_out, float *intensity_residuals_out, float *weights_out,
                                  const lsf_point_sdf_photometric_params *params, void *stream);

typedef struct lsf_point_sdf_pyramid_params {
    double fx, fy, cx, cy;             /* lsf_point_sdf_params, member for member; level 0's intrinsics */
    double depth_unit_ratio;           /* not read: the pyramid is in metres */
    double max_distance;
    double voxel_size;
    double offset_x, offset_y, offset_z;
    double narrow_band_width_voxels;
    double scale;
    int32_t depth, height, width;
    int32_t image_height, image_width; /* level 0's extents */
    int32_t depth_dtype;               /* not read: the pyramid is float32 */
    int32_t levels;                    /* tracked levels, 1 .. pyramid_levels: entry k runs on level levels - 1 - k */
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    int32_t strides[LSF_ICP_MAX_LEVELS]; /* not read */
    int32_t loss;
    double photometric_weight;         /* as lsf_point_sdf_photometric_params */
    double max_intensity_difference;
    double intensity_scale;
    int32_t pyramid_levels;            /* levels the pyramids hold, 1 .. LSF_ICP_MAX_LEVELS, the last not empty */
    int32_t reserved;
} lsf_point_sdf_pyramid_params;

/* lsf_point_sdf_run_photometric on the depth pyramid.  pyramid_depth: lsf_depth_pyramid's DEVICE float32 depth output
 * for (image_height, image_width, pyramid_levels); pyramid_intensity: NULL, or lsf_intensity_pyramid's output of the
 * frame's colour image for the same extents and levels, optional together with colour under
 * lsf_point_sdf_run_photometric's rules.  residuals_out, intensity_residuals_out, weights_out: NULL, or DEVICE float32
 * of the last iteration's level extents.  scratch: DEVICE, LSF_POINT_SDF_COLOUR_SCRATCH_BYTES.  Refused: what
 * lsf_point_sdf_run_photometric refuses (the depth type, the ratio and the strides are not read), pyramid_levels
 * outside 1 .. LSF_ICP_MAX_LEVELS, levels above pyramid_levels, a level whose extents reach 0.  sum(iterations) + 1
 * launches, none when sum(iterations) == 0; no float atomics, no host wait, a rerun is bit-identical.  No output may
 * alias an input or another output. */
int lsf_point_sdf_run_pyramid(const float *tsdf, const float *weight, const float *colour, const float *pyramid_depth,
                              const float *pyramid_intensity, double *twist_inout, double *records, void *scratch,
                              float *residuals_out, float *intensity_residuals_out, float *weights_out,
                              const lsf_point_sdf_pyramid_params *params, void *stream);

/* ---- a triangle mesh of the canonical TSDF's level set iso ------------------------------------------------------------
 * The reference has no mesh extraction; the contract is this project's ("Mesh extraction"):
 * marching cubes over the cells whose 8 corners have weight > min_weight and a finite tsdf, with the generated case
 * table of csrc/lsf_mesh_tables.h, one vertex per crossing grid edge, every float step one float64 operation.  The
 * output order is fixed (vertices by owning voxel, then axis x, y, z; faces by cell, then table order), so reruns are
 * bit-identical.  A call is lsf_mesh_count (3 launches), one host read of the two totals, then lsf_mesh_emit (2
 * launches) into outputs of exactly that size.  No inter-workgroup waits, no float atomics.
 * Workspaces (DEVICE, the caller's; voxels = depth * height * width, blocks = ceil(voxels / LSF_MESH_TILE)):
 *   cell_code      uint8 [voxels]      per cell (named by its lowest voxel): its case when valid, else 0
 *   edge_mask      uint8 [voxels]      per voxel: bit a set when its grid edge along axis a (x, y, z) has a vertex
 *   block_offsets  int32 [2][blocks]   after lsf_mesh_count: the exclusive offsets of each block's vertices ([0])
 *                                      and faces ([1])
 *   vertex_base    int32 [voxels]      lsf_mesh_emit: the index of a voxel's first vertex (where edge_mask != 0) */
typedef struct lsf_mesh_params {
    double voxel_size;                   /* metres, finite and > 0 */
    double offset_x, offset_y, offset_z; /* array offset, voxels, finite, fractional allowed */
    double iso;                          /* the level, finite; a corner is inside when (double)tsdf < iso */
    double min_weight;                   /* a voxel counts when (double)weight > min_weight; not NaN */
    int32_t depth, height, width;        /* volume extents z, y, x, >= 2 each; 3 * voxels and
                                            5 * (depth - 1)(height - 1)(width - 1) at most 2^31 - 1 */
} lsf_mesh_params;
#define LSF_MESH_TILE 2048

/* tsdf, weight: DEVICE float32 [depth][height][width], two distinct buffers, read only.  Writes cell_code, edge_mask
 * and block_offsets, and totals: DEVICE int64 [2] = (vertex count V, face count F), exact.  No buffer may alias
 * another. */
int lsf_mesh_count(const float *tsdf, const float *weight, uint8_t *cell_code, uint8_t *edge_mask,
                   int32_t *block_offsets, int64_t *totals, const lsf_mesh_params *params, void *stream);

/* After lsf_mesh_count on the same inputs and workspaces, with vertex_count and face_count its totals.  vertices: DEVICE
 * float32 [vertex_count][3], world (x, y, z) in metres.  normals: NULL, or DEVICE float32 [vertex_count][3], unit
 * normals towards larger tsdf (0 where the interpolated gradient is 0).  faces: DEVICE int32 [face_count][3], vertex
 * indices, right-hand normal towards larger tsdf.  With both counts 0 nothing is launched and the outputs may be NULL.
 * No output may alias an input or another output. */
int lsf_mesh_emit(const float *tsdf, const float *weight, const uint8_t *cell_code, const uint8_t *edge_mask,
                  const int32_t *block_offsets, int32_t *vertex_base, float *vertices, float *normals, int32_t *faces,
                  int64_t vertex_count, int64_t face_count, const lsf_mesh_params *params, void *stream);

/* After lsf_mesh_emit on the same inputs and workspaces: the colour of every vertex from a colour volume (DEVICE float32
 * [depth][height][width][4], (R, G, B, Wc) per voxel, 16-byte aligned; lsf_fusion_integrate_depth_colour's).  For the
 * vertex on the grid edge from voxel v to w with lsf_mesh_emit's float64 t = (iso - tsdf[v]) / (tsdf[w] - tsdf[v]): with
 * both colour weights > 0 each channel is C_v (1 - t) + C_w t in float64, in that order; with one, that voxel's colour;
 * with neither, the default colour (each channel 0..255).  The stored byte is floor(min(max(x, 0), 255) + 0.5), and 0 for
 * a NaN.  colours: DEVICE uint8 [vertex_count][3], row i the colour of vertex i, overlapping no input.  One launch, none
 * when vertex_count is 0; each voxel with a non-zero edge_mask writes the rows of its own one to three vertices, from
 * vertex_base: no scan, no dependence between workgroups. */
int lsf_mesh_vertex_colours(const float *tsdf, const float *colour, const uint8_t *edge_mask,
                            const int32_t *vertex_base, uint8_t *colours, int64_t vertex_count, int32_t default_red,
                            int32_t default_green, int32_t default_blue, const lsf_mesh_params *params, void *stream);

/* ---- the moving volume: the canonical model shifted by whole voxels ----------------------------------------------------
 * The reference has no moving volume; the contract is this project's ("Moving volume";
 * tests/volume_shift_restatement.py restates it).  With s = (shift_x, shift_y, shift_z), any sign,
 *     dst(v) = src(v + s)                                   where v + s lies inside the volume
 *     dst(v) = (tsdf 1, weight 0, colour record 0 0 0 0)    elsewhere
 * for tsdf, weight and, when given, the 16-byte colour record.  |s_j| >= n_j on any axis gives an all-empty
 * destination.  Values move as bits: NaNs, their payloads and -0.0 survive.  Out of place, one launch, no host wait:
 * every destination voxel is written exactly once and a source voxel that leaves is never read.  The unit of work is
 * one row (z, y) per wave, LSF_VOLUME_SHIFT_BLOCK_ROWS rows per workgroup, on at most LSF_VOLUME_SHIFT_MAX_BLOCKS
 * workgroups with a stride loop behind them. */
typedef struct lsf_volume_shift_params {
    int32_t depth, height, width;        /* volume extents z, y, x, >= 1 each; at most 2^31 - 1 voxels */
    int32_t shift_x, shift_y, shift_z;   /* whole voxels, any sign and size */
} lsf_volume_shift_params;
#define LSF_VOLUME_SHIFT_MAX_BLOCKS 2048
#define LSF_VOLUME_SHIFT_BLOCK_ROWS 4

/* tsdf, weight, out_tsdf, out_weight: DEVICE float32 [depth][height][width], 4-byte aligned.  colour, out_colour: both
 * NULL (no colour volume), or both DEVICE float32 [depth][height][width][4], 16-byte aligned.  Refused with
 * LSF_ERR_BAD_ARGUMENT: a NULL among the first four, one colour pointer NULL and the other not, a colour pointer off a
 * 16-byte boundary, extents < 1, and any source array overlapping any destination array or two destination arrays
 * overlapping; more than 2^31 - 1 voxels is LSF_ERR_BAD_DIMS. */
int lsf_volume_shift(const float *tsdf, const float *weight, const float *colour, float *out_tsdf, float *out_weight,
                     float *out_colour, const lsf_volume_shift_params *params, void *stream);

/* ---- the moving volume's brick store: what leaves the window is kept, what re-enters is written back -------------------
 * The contract is this project's ("Brick store"; tests/volume_bricks_restatement.py restates
 * it).  The world is cut into bricks of LSF_VOLUME_BRICK voxels per axis on an integer lattice.  The window's voxel
 * v = (x, y, z) is the lattice voxel g + v, g = (origin_x, origin_y, origin_z), any sign; its brick is
 * floor((g + v) / 8) per axis and its place in the brick (g + v) mod 8 >= 0.  The brick grid of a window is the box of
 * bricks it touches, floor(g_j / 8) .. floor((g_j + n_j - 1) / 8) per axis, numbered z-major (x fastest).  A brick is
 * 512 records [8][8][8] (z, y, x) of each of tsdf, weight and, when given, the 16-byte colour record, and 64 validity
 * bytes: byte r = zl * 8 + yl, bit xl.
 * With s = (shift_x, shift_y, shift_z) clamped to [-n, n] per axis, lsf_volume_shift by s makes dst(v) = src(v + s).  A
 * voxel u of the OLD window therefore LEAVES when u - s lies outside the volume (no destination voxel takes it), and a
 * voxel v of the NEW window ENTERED when v + s lies outside the volume (nothing was copied into it): the voxels that
 * entered under s are the ones that leave under -s.  A voxel HOLDS DATA when the bits of its weight
 * have any of the low 31 set: any non-zero weight, a NaN included.  Values move as 32-bit words, so NaN payloads and
 * -0.0 survive.  One wave owns one brick and lane r its x-row (zl, yl) = (r / 8, r % 8); whether a brick touches the
 * leaving / entering region is decided from its coordinate before any load; LSF_VOLUME_BRICKS_BLOCK_BRICKS bricks per
 * workgroup on at most LSF_VOLUME_BRICKS_MAX_BLOCKS workgroups with a stride loop behind them.  No atomics, no waits
 * between workgroups. */
typedef struct lsf_volume_bricks_params {
    int32_t depth, height, width;           /* window extents z, y, x, >= 1 each; at most 2^31 - 1 voxels */
    int32_t origin_x, origin_y, origin_z;   /* g: the window's voxel (0, 0, 0) on the lattice; |g_j| + n_j within int32 */
    int32_t shift_x, shift_y, shift_z;      /* whole voxels, any sign and size */
} lsf_volume_bricks_params;
#define LSF_VOLUME_BRICK 8
#define LSF_VOLUME_BRICKS_MAX_BLOCKS 2048
#define LSF_VOLUME_BRICKS_BLOCK_BRICKS 4

/* Per brick b of the grid: flags[b] = 1 when any voxel of it that lies inside the window leaves and holds data, else 0;
 * offsets[b] = the exclusive prefix sum of the flags in grid order; *total = their sum.  weight: DEVICE float32
 * [depth][height][width]; flags, offsets: DEVICE int32, one per brick of the grid; total: DEVICE int64.  Two launches
 * (the flags, then a one-workgroup scan), no host wait; the order is the grid's whatever the schedule.  Refused with
 * LSF_ERR_BAD_ARGUMENT: a NULL, extents < 1, |g_j| + n_j beyond int32, a misaligned pointer, an output overlapping the
 * weights or another output; more than 2^31 - 1 voxels or bricks is LSF_ERR_BAD_DIMS. */
int lsf_volume_bricks_count(const float *weight, int32_t *flags, int32_t *offsets, int64_t *total,
                            const lsf_volume_bricks_params *params, void *stream);

/* After lsf_volume_bricks_count with the same weight and params, and after the host has read *total into brick_count:
 * every flagged brick b writes row offsets[b] of the outputs -- out_coords [brick_count][3]: its lattice brick
 * coordinate (x, y, z); out_tsdf, out_weight [brick_count][8][8][8] and out_colour [brick_count][8][8][8][4]: for a
 * voxel that is inside the window, leaves and holds data the window's words, for every other voxel the empty voxel
 * (tsdf 1, weight 0, colour record 0 0 0 0); out_valid [brick_count][64]: a bit set exactly for the voxels of the first
 * kind.  Every word of every row is written; rows come in grid order, which is ascending (z, y, x).  A row index not
 * below brick_count is never written.  One launch, none when brick_count is 0.  colour, out_colour: both NULL or both
 * set, 16-byte aligned.  Refused as lsf_volume_bricks_count refuses, and a brick_count < 0 or above the number of bricks
 * of the grid, and any output overlapping an input or another output. */
int lsf_volume_bricks_gather(const float *tsdf, const float *weight, const float *colour, const int32_t *flags,
                             const int32_t *offsets, int64_t brick_count, int32_t *out_coords, float *out_tsdf,
                             float *out_weight, float *out_colour, uint8_t *out_valid,
                             const lsf_volume_bricks_params *params, void *stream);

/* The way back, IN PLACE: for each of the brick_count given bricks (coords [brick_count][3] and the rows in
 * lsf_volume_bricks_gather's layout) and each of its voxels that lies inside the window, is entering under
 * params->shift and has its validity bit set, the brick's words are written into tsdf, weight and colour.  Nothing else
 * is touched.  |shift_j| >= n_j on some axis makes every voxel entering: a dense volume assembled from bricks.  The
 * caller guarantees distinct coordinates; bricks outside the window's grid are skipped.  One launch, none when
 * brick_count is 0.  brick_colour, colour: both NULL or both set, 16-byte aligned.  Refused as above. */
int lsf_volume_bricks_scatter(const int32_t *coords, const float *brick_tsdf, const float *brick_weight,
                              const float *brick_colour, const uint8_t *brick_valid, int64_t brick_count, float *tsdf,
                              float *weight, float *colour, const lsf_volume_bricks_params *params, void *stream);

/* ---- the RGB-D sensor front end: lens rectification and depth-to-colour registration -----------------------------------
 * The contract is this project's ("RGB-D sensor"; tests/rgbd_restatement.py restates it).  A
 * raw depth image, taken through a lens with distortion, is registered into an IDEAL pinhole camera (the rectified colour
 * camera, or the depth camera's own matrix): every depth pixel is lifted along its undistorted ray, moved by
 * q = R p + t and splatted through a z-buffer; the raw colour image is resampled into the same ideal camera.  A pixel of
 * the result without an answer has depth 0, which every kernel that reads depth treats as "no measurement".
 * Every float step is float64, one IEEE operation each in the order written here (the library is built with
 * -ffp-contract=off).  Pixel centres lie at integer coordinates.  Distortion is OpenCV's rational model with
 * k = (k1, k2, p1, p2, k3, k4, k5, k6):
 *     r2 = x*x + y*y,  num = 1 + r2*(k1 + r2*(k2 + r2*k3)),  den = 1 + r2*(k4 + r2*(k5 + r2*k6)),
 *     dx = 2*p1*x*y + p2*(r2 + 2*x*x),  dy = p1*(r2 + 2*y*y) + 2*p2*x*y,   (products left to right)
 *     xd = x*(num/den) + dx,  yd = y*(num/den) + dy.
 * One lane per pixel on workgroups of 256 lanes along rows, at most LSF_RGBD_MAX_BLOCKS workgroups with a stride loop
 * behind them; the only atomics are unsigned minima on the z-buffer and integer sums on the record, one per workgroup
 * and non-zero count (four LDS words carry the waves' sums). */
typedef struct lsf_rgbd_params {
    double fx, fy, cx, cy;                  /* the SOURCE camera: the lens of the ray table, of the rectified image */
    double k[8];                            /* its distortion (k1, k2, p1, p2, k3, k4, k5, k6); finite */
    double out_fx, out_fy, out_cx, out_cy;  /* the ideal OUTPUT camera (register_depth, rectify_colour) */
    double rotation[9];                     /* R, row-major: q = R p + t takes depth-camera to output-camera coordinates */
    double translation[3];                  /* t, in metres */
    double depth_unit_ratio;                /* register_depth: metres per depth unit, finite and > 0 */
    int32_t height, width;                  /* the source image (the depth image; the raw colour image) */
    int32_t out_height, out_width;          /* the output image */
    int32_t max_footprint;                  /* register_depth: 1 .. LSF_RGBD_MAX_FOOTPRINT output pixels per axis */
    int32_t reserved;                       /* 0 */
} lsf_rgbd_params;
#define LSF_RGBD_UNDISTORT_ITERATIONS 10
#define LSF_RGBD_MAX_FOOTPRINT 16
#define LSF_RGBD_DEFAULT_FOOTPRINT 8
#define LSF_RGBD_MAX_BLOCKS 512
#define LSF_RGBD_RECORD_WORDS 8
#define LSF_RGBD_ZBUFFER_EMPTY 0x7f800000u

/* Once per sensor: the undistorted normalised coordinates of the source camera's pixels.  corner_rays: DEVICE float64
 * [height + 1][width + 1][2], at (u - 0.5, v - 0.5) for u in 0..width, v in 0..height; centre_rays: DEVICE float64
 * [height][width][2], at (u, v).  From xd = (u - cx) / fx, yd = (v - cy) / fy: with all eight coefficients 0 the ray is
 * (xd, yd) itself; otherwise LSF_RGBD_UNDISTORT_ITERATIONS fixed-point steps from (x, y) = (xd, yd), one step being
 * x' = (xd - dx(x, y)) * den / num, y' = (yd - dy(x, y)) * den / num with r2, num, den of (x, y), no early exit.  One
 * launch.  Reads params->fx .. k, height, width.  Refused with LSF_ERR_BAD_ARGUMENT: a NULL, extents < 1, fx or fy zero
 * or not finite, cx, cy or a coefficient not finite, a table off 8-byte alignment, overlapping tables; more than
 * 2^31 - 1 pixels (corners) is LSF_ERR_BAD_DIMS. */
int lsf_rgbd_ray_table(double *corner_rays, double *centre_rays, const lsf_rgbd_params *params, void *stream);

/* depth: DEVICE [height][width] of depth_dtype (LSF_DEPTH_*), scaled as the TSDF generators scale it (uint16 and float64
 * times the ratio in float64, float32 times float32(ratio) in float32).  corner_rays, centre_rays: lsf_rgbd_ray_table's,
 * of the depth image's extents.  zbuffer: DEVICE uint32 [out_height][out_width], workspace.  colour_valid: NULL or DEVICE
 * uint8 [out_height][out_width] (lsf_rgbd_rectify_colour's).  out_depth: DEVICE float32 [out_height][out_width], metres,
 * 0 where nothing landed.  record: DEVICE int64 [LSF_RGBD_RECORD_WORDS] = valid, behind, outside, empty, clipped,
 * written, filled, masked; exact counts.  Three launches (clear, splat, finalise), no host wait.
 * Per depth pixel: z = the scaled depth as float64; VALID when z is finite and > 0.  The centre point
 * p = (xc*z, yc*z, z) moves to q_i = ((R[i][0]*p0 + R[i][1]*p1) + R[i][2]*p2) + t[i]; the pixel is BEHIND unless
 * q_z > 0 and float32(q_z) is finite.  Each of its four corner rays, scaled by the pixel's own z, moves the same way; a
 * corner with q_z <= 0 also makes the pixel BEHIND.  Each corner projects to U = out_fx*(q_x/q_z) + out_cx, V likewise.
 * The footprint is the columns u0 <= i < u1, u0 = ceil(min U), u1 = ceil(max U), and the rows v0 <= j < v1 likewise: the
 * output pixels whose centre lies in the bounding box of the projected quad; neighbours share corners, so a continuous
 * surface leaves no gap.  A U or V that is not finite, or a bound beyond +-2147483000, makes the pixel OUTSIDE.  An
 * extent above max_footprint keeps its first max_footprint columns (rows) from the low end and the pixel is counted
 * CLIPPED.  A range that holds no pixel: EMPTY.  A range wholly off the image: OUTSIDE.  Otherwise WRITTEN: every
 * in-image pixel of the range takes the unsigned minimum of itself and the bits of float32(q_z) (positive finite floats
 * order as their bits; LSF_RGBD_ZBUFFER_EMPTY is +inf), so the result does not depend on the order and reruns are bit
 * identical.  valid = behind + outside + empty + written.  Finalise: out_depth is the z-buffer's float, 0 where it is
 * empty; FILLED counts the pixels that are not empty; where colour_valid is 0, out_depth is 0 and a filled pixel is
 * counted MASKED.
 * Refused with LSF_ERR_BAD_ARGUMENT: a NULL (but colour_valid), a bad depth_dtype, extents < 1, out_fx or out_fy zero or
 * not finite, a non-finite out_cx, out_cy, R, t or ratio, a ratio <= 0, max_footprint out of range, a table off 8-byte
 * alignment, zbuffer, out_depth or depth off their element's alignment, any overlap among the buffers; more than
 * 2^31 - 1 pixels is LSF_ERR_BAD_DIMS. */
int lsf_rgbd_register_depth(const void *depth, int32_t depth_dtype, const double *corner_rays, const double *centre_rays,
                            uint32_t *zbuffer, const uint8_t *colour_valid, float *out_depth, int64_t *record,
                            const lsf_rgbd_params *params, void *stream);

/* src: DEVICE uint8 [height][width][3], the raw image of the source camera; dst: DEVICE uint8 [out_height][out_width][3];
 * valid: DEVICE uint8 [out_height][out_width].  Output pixel (u, v) gives x = (u - out_cx)/out_fx, y likewise, (xd, yd)
 * by the source's coefficients, us = fx*xd + cx, vs = fy*yd + cy.  VALID (1) when both are finite, 0 <= us <= width - 1
 * and 0 <= vs <= height - 1; then, with u0 = floor(us), a = us - u0, u1 = min(u0 + 1, width - 1) and v0, b, v1 likewise,
 * each channel is  top = s[v0][u0]*(1 - a) + s[v0][u1]*a,  bottom = s[v1][u0]*(1 - a) + s[v1][u1]*a,
 * byte = floor((top*(1 - b) + bottom*b) + 0.5).  Otherwise the pixel is (0, 0, 0) and valid 0.  One launch.  Refused as
 * above: a NULL, extents < 1, a focal length zero or not finite, a non-finite centre or coefficient, any overlap. */
int lsf_rgbd_rectify_colour(const uint8_t *src, uint8_t *dst, uint8_t *valid, const lsf_rgbd_params *params,
                            void *stream);

/* ---- keyframe ferns: a frame's code, its distance to the stored keyframes, the nearest, the append ------------------------
 * The contract is this project's ("Tracking quality and relocalisation";
 * tests/relocaliser_restatement.py restates it), after Glocker et al., "Real-time RGB-D camera relocalization via
 * randomized ferns".  A frame is reduced to a COARSE image of block means; a fern is `decisions` threshold tests on that
 * image and gives one byte; a frame's code is `ferns` bytes; the distance of two codes is the number of ferns whose bytes
 * differ.  Every sum is an integer sum and every count an integer, so the results do not depend on any order and a rerun
 * is bit identical; there are no atomics and no host wait. */
typedef struct lsf_reloc_params {
    double depth_unit_ratio;             /* encode: metres per depth unit, finite and > 0 */
    double depth_near, depth_far;        /* encode: near and far; a pixel counts when near <= d <= far; 0 < near < far <= 64 */
    int32_t height, width;               /* encode: the frame */
    int32_t coarse_height, coarse_width; /* the coarse image; encode needs coarse_height <= height, likewise the width */
    int32_t channels;                    /* of the coarse image: 1 (depth) or 4 (depth, R, G, B) */
    int32_t ferns, decisions;            /* query: F in 1 .. LSF_RELOC_MAX_FERNS, D in 1 .. LSF_RELOC_MAX_DECISIONS */
    int32_t capacity;                    /* query: the rows the database holds, >= 1 */
    int32_t candidates;                  /* query: 1 .. LSF_RELOC_MAX_CANDIDATES nearest keyframes */
    int32_t harvest;                     /* query: 1 appends the frame when it is far from every keyframe, 0 never */
    int32_t harvest_differing;           /* query with harvest: the least distance that appends, >= 1 */
    int32_t reserved;                    /* 0 */
} lsf_reloc_params;
#define LSF_RELOC_MAX_BLOCKS 1024
#define LSF_RELOC_MAX_FERNS 4096
#define LSF_RELOC_MAX_DECISIONS 8
#define LSF_RELOC_MAX_CANDIDATES 4
#define LSF_RELOC_MAX_DEPTH 64.0
#define LSF_RELOC_ENCODE_RECORD_WORDS 2
#define LSF_RELOC_QUERY_RECORD_WORDS 12

/* depth: DEVICE [height][width] of depth_dtype (LSF_DEPTH_*), scaled as the TSDF generators scale it (uint16 and float64
 * times the ratio in float64, float32 times float32(ratio) in float32); d is that value as float64.  colour: NULL
 * (channels 1) or DEVICE uint8 [height][width][3] registered to the depth (channels 4).  coarse: DEVICE float32
 * [coarse_height][coarse_width][channels].  block_counts: DEVICE int32 [coarse_height][coarse_width], the counting pixels
 * of every block.  record: DEVICE int32 [LSF_RELOC_ENCODE_RECORD_WORDS] = counting pixels, valid blocks.
 * Coarse row i covers the image rows [i*height/coarse_height, (i + 1)*height/coarse_height) in integer division, the
 * columns likewise.  A pixel COUNTS when near <= d <= far (a NaN does not).  A block is VALID when at least half of its
 * pixels count (2*count >= pixels).  A valid block's depth is float32((double(sum q) / double(count)) / 2^20) with
 * q = (int64) rint(d * 2^20) summed as integers over its counting pixels, and with colour its channels 1..3 are
 * float32(double(sum of the byte) / double(count)) over the same pixels; every channel of a block that is not valid is 0.
 * Two launches (a wave per block; one workgroup for the record).  Refused with LSF_ERR_BAD_ARGUMENT: a NULL (but
 * colour), a bad depth_dtype, extents < 1, a coarse extent above the image's, channels that is not 1 without and 4 with
 * colour, a ratio, near or far that is not finite, ratio <= 0, near <= 0, near >= far, far > LSF_RELOC_MAX_DEPTH, a buffer
 * off its element's alignment, any overlap; more than 2^31 - 1 pixels is LSF_ERR_BAD_DIMS. */
int lsf_reloc_encode(const void *depth, int32_t depth_dtype, const uint8_t *colour, float *coarse, int32_t *block_counts,
                     int32_t *record, const lsf_reloc_params *params, void *stream);

/* coarse: lsf_reloc_encode's.  The fern table, DEVICE, [ferns][decisions] each: locations int32 (a coarse pixel index
 * i*coarse_width + j), channels uint8 (< channels), thresholds float32.  codes: DEVICE uint8 [capacity][ferns], 16-byte
 * aligned, the database; n_keyframes: DEVICE int32, its size, read as min(max(n, 0), capacity).  frame_code: DEVICE uint8
 * [ferns], out.  distances: DEVICE int32 [capacity], out.  record: DEVICE int32 [LSF_RELOC_QUERY_RECORD_WORDS], out.
 * Frame code: bit j of byte f is 1 when coarse[location][channel] > threshold AND coarse[location][0] > 0, for decision
 * (f, j); a location or a channel outside the coarse image gives 0.  distances[k] for k < n: the ferns f with
 * codes[k][f] != frame_code[f]; -1 for k >= n.  Nearest: the `candidates` keyframes in rising order of (distance, id).
 * With harvest, the frame is WANTED when n == 0 or the smallest distance is >= harvest_differing; a wanted frame is
 * appended when n < capacity: codes[n] = frame_code and *n_keyframes = n + 1 (distances keeps the values from before).
 * *n_keyframes is written only by an append, n being the value as read: a word below 0 becomes 1 when the frame is
 * appended (an empty database wants every frame) and stays as it was otherwise; a word above capacity is never written,
 * and a wanted frame sets record[10].
 * record: [0] n before the call, [1, 5) the nearest ids, -1 where n is smaller, [5, 9) their distances, -1 likewise,
 * [9] the appended id or -1, [10] 1 when a wanted frame met a full database, [11] 0.
 * Three launches (the code; a wave per keyframe row, which reads aligned 16-byte words; one workgroup that selects and
 * appends).  Refused with LSF_ERR_BAD_ARGUMENT: a NULL, coarse extents < 1, channels not 1 or 4, ferns, decisions or
 * candidates out of range, capacity < 1, harvest not 0 or 1, harvest_differing < 1 with harvest, codes off 16-byte and
 * an int32 or float32 buffer off 4-byte alignment, any overlap; capacity * ferns above 2^31 - 1 is LSF_ERR_BAD_DIMS. */
int lsf_reloc_query(const float *coarse, const int32_t *locations, const uint8_t *channels, const float *thresholds,
                    uint8_t *codes, int32_t *n_keyframes, uint8_t *frame_code, int32_t *distances, int32_t *record,
                    const lsf_reloc_params *params, void *stream);

/* ---- mesh simplification: welding and vertex-clustering decimation of a triangle mesh ----------------------------------
 * The reference has no mesh at all; the contract is this project's ("Mesh simplification";
 * tests/mesh_simplify_restatement.py restates it).  Vertices are grouped by a key -- the three bit patterns of the
 * position with -0 read as +0 (weld), or the cell floor((p - origin) / cell_size) of a lattice (cluster) --, every group
 * becomes one vertex, the faces are remapped, and faces that collapse, fold onto each other or repeat are dropped.
 * Groups are found with an open-addressing hash table claimed by integer compare-and-swap; every sum is an integer
 * atomic, so no output depends on which lane wins a slot or on the order lanes run in: a rerun, and a run with another
 * table_slots, is bit-identical.  A call is lsf_mesh_simplify_count, one host read of the record, then
 * lsf_mesh_simplify_emit into outputs of exactly the record's sizes.  Every probe loop ends after table_slots steps.
 * Workspaces (DEVICE, the caller's, uninitialised; V = vertex_count, F = face_count, blocks(n) = ceil(n /
 * LSF_MESH_SIMPLIFY_TILE), K = 3 * (cluster + has_normals + has_colours)):
 *   table          int32 [table_slots]                          the hash table, used for the vertices, then the faces
 *   vertex_work    int32 [LSF_MESH_SIMPLIFY_VERTEX_WORDS][V]    key (3 planes, [V][3]), slot, cluster id
 *   cluster_work   int32 [LSF_MESH_SIMPLIFY_CLUSTER_WORDS][V]   members, used, first member, output index
 *   sums           int64 [V][K]                                 per cluster: sum q (cluster), sum m (normals), sum c
 *   face_work      int32 [LSF_MESH_SIMPLIFY_FACE_WORDS][F]      sorted ids (3 planes, [F][3]), state, net, first + / -
 *   tile_offsets   int32 [3 * blocks(V) + 3 * blocks(F)]        the three scans' tile counts, then exclusive offsets,
 *                                                               and the tiles' statistics words */
typedef struct lsf_mesh_simplify_params {
    double cell_size;                    /* cluster: the lattice edge, finite and > 0; weld: not read */
    double origin_x, origin_y, origin_z; /* the lattice origin, finite; weld: not read */
    int32_t vertex_count, face_count;    /* V and F, each 0 .. LSF_MESH_SIMPLIFY_MAX_ITEMS */
    int32_t table_slots;                 /* a power of two, >= 2 * max(V, F, 1) */
    int32_t cluster;                     /* 0: weld by bit pattern; 1: cluster by lattice cell */
    int32_t has_normals, has_colours;    /* 0 or 1: whether normals / colours are given and produced */
} lsf_mesh_simplify_params;
#define LSF_MESH_SIMPLIFY_TILE 256
#define LSF_MESH_SIMPLIFY_SCAN_THREADS 256
#define LSF_MESH_SIMPLIFY_MAX_ITEMS (1 << 29)
#define LSF_MESH_SIMPLIFY_VERTEX_WORDS 5
#define LSF_MESH_SIMPLIFY_CLUSTER_WORDS 4
#define LSF_MESH_SIMPLIFY_FACE_WORDS 7
/* the record, DEVICE int64 [LSF_MESH_SIMPLIFY_RECORD_WORDS]: vertices_in, faces_in, invalid_vertices, invalid_faces,
 * clusters, degenerate_faces, face_groups, cancelled_groups, multi_cover_groups, orphan_clusters, vertices_out,
 * faces_out, table_overflow */
#define LSF_MESH_SIMPLIFY_RECORD_WORDS 13

/* vertices: DEVICE float32 [V][3]; faces: DEVICE int32 [F][3], any values (an index outside [0, V) makes the face
 * invalid; it is checked before any gather); normals: DEVICE float32 [V][3] with has_normals, else NULL; colours: DEVICE
 * uint8 [V][3] with has_colours, else NULL; all read only.  Writes the workspaces and the record.  Six fills and thirteen
 * launches at most, no host wait.  Refused with LSF_ERR_BAD_ARGUMENT: a NULL where a size is not 0, a count outside its
 * range, a table_slots that is not a power of two or is below 2 * max(V, F, 1), a flag that is not 0 or 1, normals or
 * colours against their flag, in cluster mode a cell_size that is not finite and > 0 or an origin that is not finite,
 * any overlap. */
int lsf_mesh_simplify_count(const float *vertices, const int32_t *faces, const float *normals, const uint8_t *colours,
                            int32_t *table, int32_t *vertex_work, int32_t *cluster_work, int64_t *sums,
                            int32_t *face_work, int32_t *tile_offsets, int64_t *record,
                            const lsf_mesh_simplify_params *params, void *stream);

/* After lsf_mesh_simplify_count on the same inputs, workspaces and params, with clusters, vertices_out and faces_out the
 * record's.  out_vertices: DEVICE float32 [vertices_out][3]; out_normals: DEVICE float32 [vertices_out][3] with
 * has_normals, else NULL; out_colours: DEVICE uint8 [vertices_out][3] with has_colours, else NULL; out_faces: DEVICE int32
 * [faces_out][3].  Two launches at most, none when vertices_out is 0.  Refused: what lsf_mesh_simplify_count refuses,
 * clusters outside 0 .. V, vertices_out outside 0 .. clusters, faces_out outside 0 .. F, faces without vertices, a NULL
 * output of a size that is not 0, any overlap. */
int lsf_mesh_simplify_emit(const float *vertices, const int32_t *faces, const int32_t *vertex_work,
                           int32_t *cluster_work,
                           const int64_t *sums, const int32_t *face_work, const int32_t *tile_offsets,
                           float *out_vertices, float *out_normals, uint8_t *out_colours, int32_t *out_faces,
                           int64_t clusters, int64_t vertices_out, int64_t faces_out,
                           const lsf_mesh_simplify_params *params, void *stream);

/* ---- mesh components: connected components of a triangle mesh, and the filter that removes components ------------------
 * The reference has no mesh at all; the contract is this project's ("Mesh components";
 * tests/mesh_components_restatement.py restates it).  Two vertices are connected when some face names both (a degenerate
 * face still connects what it names); a component is a connected set of vertices, a vertex no face names is one of its
 * own with 0 faces.  A component's label is the smallest vertex index in it, a face's label the label of its first
 * vertex: the answer is a function of the mesh alone.  The table lists the C components in ascending label order with
 * their vertex and face counts and bounds, the componentwise minimum and maximum of the members' positions (-0 read as
 * +0).  The filter keeps the vertices and faces of the components whose row of keep[] is not 0, in input order, faces
 * re-indexed, normals and colours carried bit for bit.
 * Labels come from a lock-free union-find over parent[V] with integer atomics only: a root is linked under a smaller
 * index of the other set by compare-and-swap, so a parent is always a strictly smaller index, every walk is strictly
 * decreasing and the final root is the component's minimum, whichever lane wins.  Inside the linking launch every read
 * of parent[] is a device-scope atomic load or the value a failed compare-and-swap returned.  Every walk and every retry
 * loop ends after V + 1 steps at the latest (a walk takes at most V, and a compare-and-swap fails only because one of the
 * at most V - 1 links succeeded); a lane that gets there adds to the record's step_cap and stops.  Counts and bounds are
 * integer atomics (the bounds through an order-preserving image of the float bits), rows and kept items come from scans
 * over index order: a rerun, and a run with another max_blocks, is bit-identical.
 * A call is lsf_mesh_components_label, a host read of the record (components), then lsf_mesh_components_table into
 * outputs of exactly that size; the filter goes on with lsf_mesh_components_select, a second host read of the record
 * (vertices_out, faces_out) and lsf_mesh_components_emit into outputs of exactly those sizes.
 * Every launch but the one-workgroup scans walks tiles of LSF_MESH_COMPONENTS_TILE items on a grid of at most max_blocks
 * workgroups with a stride loop behind it; the scan workgroup of LSF_MESH_COMPONENTS_SCAN_THREADS lanes loops over the
 * tile counts.
 * Workspaces (DEVICE, the caller's, uninitialised; V = vertex_count, F = face_count, tiles(n) = ceil(n /
 * LSF_MESH_COMPONENTS_TILE)):
 *   vertex_work    int32 [LSF_MESH_COMPONENTS_VERTEX_WORDS][V]   parent, label, and indexed by label: vertex count, face
 *                                                                count, bounds images (3 minima, 3 maxima), table row;
 *                                                                then the output index of the vertex
 *   tile_offsets   int32 [3 * tiles(V) + tiles(F)]               the scans' tile counts, then exclusive offsets */
typedef struct lsf_mesh_components_params {
    int32_t vertex_count, face_count; /* V and F, each 0 .. LSF_MESH_COMPONENTS_MAX_ITEMS */
    int32_t has_normals, has_colours; /* 0 or 1: whether lsf_mesh_components_emit carries normals / colours */
    int32_t max_blocks;               /* the cap of every grid, 1 .. LSF_MESH_COMPONENTS_MAX_BLOCKS; 0: that maximum.
                                         No output depends on it */
} lsf_mesh_components_params;
#define LSF_MESH_COMPONENTS_TILE 256
#define LSF_MESH_COMPONENTS_SCAN_THREADS 256
#define LSF_MESH_COMPONENTS_MAX_BLOCKS 512
#define LSF_MESH_COMPONENTS_MAX_ITEMS (1 << 29)
#define LSF_MESH_COMPONENTS_VERTEX_WORDS 12
/* the record, DEVICE int64 [LSF_MESH_COMPONENTS_RECORD_WORDS]: vertices_in, faces_in, invalid_vertices (a non-finite
 * coordinate), invalid_faces (an index outside [0, V)), components, step_cap (lanes that met a step cap: never, by the
 * argument above), and written by lsf_mesh_components_select: components_kept, vertices_out, faces_out */
#define LSF_MESH_COMPONENTS_RECORD_WORDS 9

/* vertices: DEVICE float32 [V][3]; faces: DEVICE int32 [F][3], any values (a face with an index outside [0, V) is counted
 * before any gather and links nothing); both read only.  Writes the workspaces and the record (components_kept,
 * vertices_out and faces_out as 0).  Seven launches at most, no fill, no host wait.  A caller refuses the mesh when the
 * record counts an invalid vertex or face, and treats step_cap != 0 as an error.  Refused with LSF_ERR_BAD_ARGUMENT: a
 * NULL where a size is not 0, a count outside its range, max_blocks outside its range, a flag that is not 0 or 1, a buffer
 * off 4-byte (the record: 8-byte) alignment, any overlap. */
int lsf_mesh_components_label(const float *vertices, const int32_t *faces, int32_t *vertex_work, int32_t *tile_offsets,
                              int64_t *record, const lsf_mesh_components_params *params, void *stream);

/* After lsf_mesh_components_label on the same faces, vertex_work and params, with components the record's.  labels,
 * vertex_counts, face_counts: DEVICE int32 [components]; bounds: DEVICE float32 [components][2][3] (minimum, maximum);
 * face_labels: DEVICE int32 [F].  The vertex labels are plane 1 of vertex_work.  Two launches at most.  Refused: what
 * lsf_mesh_components_label refuses, components outside 0 .. V or 0 with V > 0. */
int lsf_mesh_components_table(const int32_t *faces, const int32_t *vertex_work, int32_t *labels, int32_t *vertex_counts,
                              int32_t *face_counts, float *bounds, int32_t *face_labels, int64_t components,
                              const lsf_mesh_components_params *params, void *stream);

/* After lsf_mesh_components_label likewise.  keep: DEVICE int32 [components], not 0 where the component of that row of
 * the table stays; read only.  Counts the kept components, vertices and faces into the record and leaves the kept items'
 * tile offsets in tile_offsets.  One fill and four launches at most, no host wait.  Refused: as above. */
int lsf_mesh_components_select(const int32_t *faces, const int32_t *vertex_work, const int32_t *keep,
                               int32_t *tile_offsets, int64_t *record, int64_t components,
                               const lsf_mesh_components_params *params, void *stream);

/* After lsf_mesh_components_select on the same inputs, workspaces, keep and params, with vertices_out and faces_out the
 * record's.  normals: DEVICE float32 [V][3] with has_normals, else NULL; colours: DEVICE uint8 [V][3] with has_colours,
 * else NULL.  out_vertices: DEVICE float32 [vertices_out][3]; out_normals, out_colours likewise with their flags, else
 * NULL; out_faces: DEVICE int32 [faces_out][3].  Two launches at most, none when vertices_out is 0.  Refused: as above,
 * vertices_out outside 0 .. V, faces_out outside 0 .. F, faces without vertices, normals or colours against their flag. */
int lsf_mesh_components_emit(const float *vertices, const int32_t *faces, const float *normals, const uint8_t *colours,
                             int32_t *vertex_work, const int32_t *keep, const int32_t *tile_offsets,
                             float *out_vertices, float *out_normals, uint8_t *out_colours, int32_t *out_faces,
                             int64_t components, int64_t vertices_out, int64_t faces_out,
                             const lsf_mesh_components_params *params, void *stream);

/* ---- mesh smoothing: Taubin passes over the edge neighbours, and vertex normals rebuilt from the faces -------------------
 * The reference has no mesh at all; the contract is this project's ("Mesh smoothing";
 * tests/mesh_smooth_restatement.py restates it and the kernels equal it bit for bit at any launch shape and table size).
 * Edges: every face contributes its corner pairs (0,1), (1,2), (2,0); a pair with equal ends is skipped, every other pair
 * adds 1 to the face count of the undirected edge {a, b} (a face naming a vertex twice adds 2 to its one edge).  Two
 * vertices are neighbours when an edge joins them; N(i) is the set of distinct neighbours, d(i) its size.
 * Pinned: with boundary_fixed a vertex is pinned when it is an end of an edge whose face count is not 2 (open borders and
 * non-manifold edges); otherwise none is.  A pinned vertex and a vertex with d = 0 keep their position bit for bit.
 * One pass with weight w (lambda or mu, float64): B is the largest |coordinate| of the pass's input, by an integer maximum
 * on the float bits; with E the exponent field of B's bits, e = max(E, 1) - 126 (B < 2^e, and B >= 2^(e-1) for a normal
 * B), q = 2^(e-32), and q = 1 when B = 0.  Q(x) = (int64) rint(double(x) / q), ties to even, 0 for a non-finite x (q and
 * 1 / q are powers of two and x / q stays a normal double, so the kernels multiply by 1 / q: the same bits).
 * S_i = sum over j in N(i) of Q(p_j) per axis, in integers: no order of the sum can matter.
 * m = (double(S_i) * q) / double(d(i));  p_i' = float32(double(p_i) + w * (m - double(p_i))), every float64 operation
 * rounded on its own.  An iteration is a lambda pass, then a mu pass when mu != 0; positions are float32 between passes;
 * each pass takes B from its own input, which the pass before leaves behind as a wave-reduced integer maximum.
 * Vertex normals: for a face (a, b, c) with u = double(p_b) - double(p_a), v = double(p_c) - double(p_a) the vector
 * c = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x), every operation rounded on its own (the right-hand normal,
 * extract_mesh's "towards larger tsdf").  M is the largest |component| over all faces, by an integer maximum on the doubles'
 * bits; with E the exponent field of M's bits, em = max(E, 1) - 1022 (M < 2^em), qn = 2^(em-32), and qn = 1 when M = 0.
 * Every face adds (int64) rint(c / qn), 0 for a non-finite component, to its three vertices by integer atomics.  With S
 * the float64 of a vertex's sums and L = sqrt((S_x^2 + S_y^2) + S_z^2) the normal is float32(S / L), and (0, 0, 0) when
 * L = 0, which the record counts.
 * Loops and their bounds: a probe walk of the edge table ends after table_slots steps (table_overflow counts a pair that
 * found no slot: never, while table_slots >= 2 * 3F); a vertex's gather walks its row of d(i) <= 2E neighbours and never
 * past the neighbour list's 6F words.  No float atomics, no inter-workgroup waits.  Every launch but the one-workgroup scan
 * walks tiles of LSF_MESH_SMOOTH_TILE items on a grid of at most max_blocks workgroups with a stride loop behind it.
 * Workspaces (DEVICE, the caller's, uninitialised; V = vertex_count, F = face_count, tiles(n) = ceil(n / LSF_MESH_SMOOTH_TILE)):
 *   vertex_work   int32 [LSF_MESH_SMOOTH_VERTEX_WORDS][V]   degree, pinned, row offset, fill cursor
 *   edge_keys     int64 [table_slots]                       the open-addressing table: (lo << 32) | hi, or -1
 *   edge_counts   int32 [table_slots]                       faces per edge
 *   tile_offsets  int32 [tiles(V)]                          the degree scan's tile counts, then exclusive offsets
 *   neighbours    int32 [max(6F, 1)]                        the compressed-row neighbour list
 *   scalars       int64 [LSF_MESH_SMOOTH_SCALAR_WORDS]      B's bits of the input, three rotating words for the passes'
 *                                                           maxima, M's bits */
typedef struct lsf_mesh_smooth_params {
    int32_t vertex_count, face_count; /* V and F, each 0 .. LSF_MESH_SMOOTH_MAX_ITEMS */
    int32_t table_slots;              /* a power of two, 2 * max(3F, 1) .. LSF_MESH_SMOOTH_MAX_SLOTS.  No output depends
                                         on it */
    int32_t boundary_fixed;           /* 0 or 1: whether the ends of an edge whose face count is not 2 are pinned */
    int32_t fresh_record;             /* 0 or 1, lsf_mesh_vertex_normals only: 1 for a call on its own, which begins the
                                         record and counts invalid vertices and faces; 0 after lsf_mesh_smooth_prepare,
                                         whose record it keeps and completes */
    int32_t iterations;               /* 0 .. LSF_MESH_SMOOTH_MAX_ITERATIONS */
    int32_t max_blocks;               /* the cap of every grid, 1 .. LSF_MESH_SMOOTH_MAX_BLOCKS; 0: that maximum.  No
                                         output depends on it */
    int32_t reserved;                 /* 0 */
    double lam, mu;                   /* lambda: finite, in (0, 1]; mu: finite, <= 0, and 0 leaves the mu passes out */
} lsf_mesh_smooth_params;
#define LSF_MESH_SMOOTH_TILE 256
#define LSF_MESH_SMOOTH_SCAN_THREADS 256
#define LSF_MESH_SMOOTH_MAX_BLOCKS 512
#define LSF_MESH_SMOOTH_MAX_ITEMS (1 << 27)
#define LSF_MESH_SMOOTH_MAX_SLOTS (1 << 30)
#define LSF_MESH_SMOOTH_MAX_ITERATIONS 1000
#define LSF_MESH_SMOOTH_VERTEX_WORDS 4
#define LSF_MESH_SMOOTH_SCALAR_WORDS 5
/* the record, DEVICE int64 [LSF_MESH_SMOOTH_RECORD_WORDS]: vertices_in, faces_in, invalid_vertices (a non-finite
 * coordinate), invalid_faces (an index outside [0, V)), edges, boundary_edges (face count 1), nonmanifold_edges (face
 * count > 2), pinned_vertices, isolated_vertices (d = 0), max_degree, table_overflow, and written by lsf_mesh_smooth_run:
 * nonfinite_out (the non-finite coordinates the last pass wrote), by lsf_mesh_vertex_normals: zero_normals */
#define LSF_MESH_SMOOTH_RECORD_WORDS 13

/* vertices: DEVICE float32 [V][3]; faces: DEVICE int32 [F][3], any values (a face with an index outside [0, V) is counted
 * before any gather and contributes no edge); both read only.  Writes every workspace and the whole record.  Two fills and
 * eight launches at most, no host wait.  A caller refuses the mesh when the record counts an invalid vertex or face, and
 * treats table_overflow != 0 as an error.  Refused with LSF_ERR_BAD_ARGUMENT, before any launch: a NULL where a size is not
 * 0, a count, table_slots, iterations or max_blocks outside its range, a table_slots that is no power of two, a flag that
 * is not 0 or 1, reserved not 0, lam or mu outside its range, a buffer off 4-byte (int64 buffers: 8-byte) alignment, any
 * overlap. */
int lsf_mesh_smooth_prepare(const float *vertices, const int32_t *faces, int32_t *vertex_work, int64_t *edge_keys,
                            int32_t *edge_counts, int32_t *tile_offsets, int32_t *neighbours, int64_t *scalars,
                            int64_t *record, const lsf_mesh_smooth_params *params, void *stream);

/* After lsf_mesh_smooth_prepare on the same vertices, workspaces and params.  The passes run ping-pong between
 * out_vertices and scratch (DEVICE float32 [V][3] each), the first reading vertices, the last writing out_vertices; one
 * small launch and one launch per pass: iterations passes when mu = 0, else twice as many.  iterations = 0 copies the
 * positions.  Writes the record's nonfinite_out.  Refused: as above. */
int lsf_mesh_smooth_run(const float *vertices, const int32_t *vertex_work, const int32_t *neighbours, float *out_vertices,
                        float *scratch, int64_t *scalars, int64_t *record, const lsf_mesh_smooth_params *params,
                        void *stream);

/* The area-weighted vertex normals of any mesh.  vertices, faces as above; sums: DEVICE int64 [V][3], a workspace;
 * normals: DEVICE float32 [V][3].  One fill and four launches (five with fresh_record), none when V = 0 and the record is
 * kept.  Writes the record's zero_normals, and with fresh_record the whole record (the smoothing's words as 0).
 * Refused: as above. */
int lsf_mesh_vertex_normals(const float *vertices, const int32_t *faces, int64_t *sums, float *normals, int64_t *scalars,
                            int64_t *record, const lsf_mesh_smooth_params *params, void *stream);

/* ---- Euclidean distance field: the exact, capped distance transform of the model's zero crossing ------------------------
 * The reference has no distance transform; the contract is this project's ("Euclidean distance
 * field"; tests/esdf_restatement.py restates it).  observed(v): weight(v) > min_weight.  inside(v): observed and
 * tsdf(v) < iso.  site(v): observed, and some in-bounds 6-neighbour is observed with the other inside flag; with
 * unknown = LSF_ESDF_UNKNOWN_OCCUPIED every voxel that is not observed is a site too.  key(v) = min over the sites s of
 * (|v - s|^2, flat(s)), compared lexicographically, flat(s) = (z Y + y) X + x.  With R = max_distance_voxels:
 *   distance2   the key's first part where it is <= R^2, else LSF_ESDF_FAR
 *   nearest     the key's second part, -1 where distance2 is LSF_ESDF_FAR
 *   esdf        sign * (sqrtf((float)distance2) * (float)voxel_size), (float)R in place of the root where distance2 is
 *               LSF_ESDF_FAR; sign is -1 where inside(v), else +1
 * The key is separable: a pass along x (which also finds the sites), one along y, one along z, each a partial minimum
 * within R of the voxel, integers throughout.  No output depends on the launch shape: a rerun is bit-identical.
 * Every launch walks a grid capped at LSF_ESDF_MAX_BLOCKS workgroups with a stride loop behind it: the x pass a row
 * (z, y) per wave, LSF_ESDF_BLOCK_ROWS rows per workgroup, the y and z passes a voxel per lane, LSF_ESDF_BLOCK_VOXELS
 * per workgroup.  Every loop is bounded by the volume's extents and by R. */
typedef struct lsf_esdf_params {
    double voxel_size;           /* metres, finite and > 0; rounded to float32 before the one multiply */
    float iso, min_weight;       /* not NaN */
    int32_t depth, height, width; /* Z, Y, X: each >= 1, Z Y X <= 2^31 - 1 */
    int32_t max_distance_voxels; /* R: 1 .. LSF_ESDF_MAX_DISTANCE */
    int32_t unknown;             /* LSF_ESDF_UNKNOWN_FREE or LSF_ESDF_UNKNOWN_OCCUPIED */
    int32_t passes;              /* which launches the call enqueues, in order x, y, z: LSF_ESDF_PASSES_ALL, or for
                                    measurement any non-empty subset, over the scratch a full call left */
} lsf_esdf_params;
#define LSF_ESDF_UNKNOWN_FREE 0
#define LSF_ESDF_UNKNOWN_OCCUPIED 1
#define LSF_ESDF_PASS_X 1
#define LSF_ESDF_PASS_Y 2
#define LSF_ESDF_PASS_Z 4
#define LSF_ESDF_PASSES_ALL 7
#define LSF_ESDF_MAX_DISTANCE 4096
#define LSF_ESDF_FAR 0x7fffffff
#define LSF_ESDF_MAX_BLOCKS 2048
#define LSF_ESDF_BLOCK_ROWS 4
#define LSF_ESDF_BLOCK_VOXELS 256
/* the record, DEVICE int64 [LSF_ESDF_RECORD_WORDS]: sites, finite (voxels whose distance2 is not LSF_ESDF_FAR),
 * max_distance2 (the largest such distance2; 0 when there is none).  Exact counts. */
#define LSF_ESDF_RECORD_WORDS 3

/* tsdf, weight: DEVICE float32 [Z][Y][X], read only.  scratch_a, scratch_b: DEVICE int32 [Z][Y][X], the caller's,
 * uninitialised (the x pass leaves each voxel's signed offset to its row's nearest site in scratch_b, the y pass the
 * packed offsets within the plane in scratch_a).  distance2, nearest: DEVICE int32 [Z][Y][X]; esdf: DEVICE float32
 * [Z][Y][X]; record as above.  One fill (the record, zeroed by every call), then at most three launches;
 * no host wait.  Refused with LSF_ERR_BAD_ARGUMENT before anything is launched: a NULL pointer, a dimension < 1, R outside
 * 1 .. LSF_ESDF_MAX_DISTANCE, a voxel_size that is not finite and > 0, a NaN iso or min_weight, an unknown code other than
 * the two, passes outside 1 .. LSF_ESDF_PASSES_ALL, a buffer off 4-byte (the record: 8-byte) alignment, any overlap
 * between an output or scratch buffer and any other buffer; with LSF_ERR_BAD_DIMS: more than 2^31 - 1 voxels. */
int lsf_esdf_compute(const float *tsdf, const float *weight, int32_t *scratch_a, int32_t *scratch_b,
                     int32_t *distance2, int32_t *nearest, float *esdf, int64_t *record,
                     const lsf_esdf_params *params, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSF_HIP_H */
