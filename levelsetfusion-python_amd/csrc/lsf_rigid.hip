// SDF-2-SDF rigid 2-D tracker (reference rigid_opt/sdf_2_sdf_optimizer2d.py:60-137, rigid_opt/sdf_gradient_field.py:
// 13-38, math_utils/transformation.py:11-34).  One kernel, three modes:
//   GRADIENT  calculate_gradient_wrt_twist of a given live field and twist (one launch)
//   ITERATE   iteration k of optimize(): prologue = combine iteration k-1's per-block partial sums (fixed order, the
//             same in every block), singular test, 3x3 solve and update -- every block computes the same twist bit for
//             bit, block 0 writes record k-1; body = regenerate the live TSDF of a 16 x 16 tile plus a one-voxel halo
//             in LDS under the pose, np.gradient, twist gradient, and the 10 float64 sums of A, b and the energy,
//             reduced through the wave and the block into this block's partial (ping-pong buffer k & 1)
//   FINISH    the prologue alone for the last iteration, one block; writes the final twist
// The partials cross a launch boundary only (cdna_hip_programming.md, split-K item 2, the launch-boundary reduce): no
// atomics, no in-launch hand-off, so a run is bit-reproducible.  Per-voxel arithmetic follows the reference's dtypes
// (tests/rigid_restatement.py) and is bit-identical to the restatement under -ffp-contract=off; the sums are tree
// reductions, not the reference's sequential loop.
#include "lsf_device.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kRT = 16;          // tile edge: 16 x 16 voxels = one thread each
constexpr int kRH = kRT + 2;     // with the one-voxel halo
constexpr int kSums = 10;        // A (6: 00 01 02 11 12 22), b (3), energy
constexpr int kRec = LSF_RIGID_RECORD_DOUBLES;
constexpr int kMaxBlocks = LSF_RIGID_MAX_BLOCKS;
static_assert(kBlock == kRT * kRT, "one thread per tile voxel");
static_assert(kMaxBlocks <= kBlock, "the prologue gives every partial one thread");

enum Mode { GRADIENT = 0, ITERATE = 1, FINISH = 2 };

struct RigidDev {
    TypedTsdf t;
    double voxel_size;  // the gradient's voxel size (p.t.voxel_size is the generator's)
    double twist[3];    // GRADIENT
    double rate;
    float eta;
    float voxel_size_f;
    int h, w, tiles_x, tiles;
    int nblocks;      // ITERATE launches' grid: the number of partials
};

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of v[] over the block in a fixed order; the totals land in thread 0's v[]
__device__ inline void block_sum(double (&v)[kSums], double (*red)[kSums]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < kSums; ++c) v[c] = wave_sum(v[c]);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < kSums; ++c) red[wave][c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < kSums; ++c) {
            double s = red[0][c];
            for (int q = 1; q < kBlock / kWave; ++q) s += red[q][c];
            v[c] = s;
        }
    __syncthreads();
}

// 3x3 inverse by LU with partial pivoting (LAPACK getrf/getri's pivot rule: first largest magnitude); false on an exact
// zero pivot -- A == 0, a zero row and column (a twist-gradient component that is 0 at every voxel), or any other A the
// elimination finds exactly singular: the cases where the reference's np.linalg.cond(A) is inf and it skips the update
__device__ inline bool invert3(const double a[9], double inv[9]) {
    double m[3][3];
    int perm[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = a[i * 3 + j];
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        for (int r = c + 1; r < 3; ++r)
            if (fabs(m[r][c]) > fabs(m[piv][c])) piv = r;
        if (m[piv][c] == 0.0) return false;
        if (piv != c) {
            for (int j = 0; j < 3; ++j) { const double t = m[c][j]; m[c][j] = m[piv][j]; m[piv][j] = t; }
            const int t = perm[c]; perm[c] = perm[piv]; perm[piv] = t;
        }
        for (int r = c + 1; r < 3; ++r) {
            m[r][c] = m[r][c] / m[c][c];
            for (int j = c + 1; j < 3; ++j) m[r][j] = m[r][j] - m[r][c] * m[c][j];
        }
    }
    for (int col = 0; col < 3; ++col) {  // solve L U x = P e_col
        double y[3];
        for (int i = 0; i < 3; ++i) {
            double s = perm[i] == col ? 1.0 : 0.0;
            for (int j = 0; j < i; ++j) s = s - m[i][j] * y[j];
            y[i] = s;
        }
        for (int i = 2; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < 3; ++j) s = s - m[i][j] * inv[j * 3 + col];
            inv[i * 3 + col] = s / m[i][i];
        }
    }
    return true;
}

// combine iteration k-1 (partials in scratch buffer (k-1) & 1, twist before it in `prev`), update, write record k-1
// (block 0); the new twist goes to tw_out (LDS) for every thread
__device__ void combine_and_update(const RigidDev& p, int k, const double* __restrict__ prev, double* __restrict__ records,
                                   const double* __restrict__ scratch, double (*red)[kSums], double* tw_out,
                                   double* twist_final) {
    double v[kSums];
    const double* part = scratch + (size_t)((k - 1) & 1) * kMaxBlocks * kSums;
#pragma unroll
    for (int c = 0; c < kSums; ++c) v[c] = 0.0;
    if ((int)threadIdx.x < p.nblocks)
#pragma unroll
        for (int c = 0; c < kSums; ++c) v[c] = part[threadIdx.x * kSums + c];
    block_sum(v, red);
    if (threadIdx.x == 0) {
        const double a[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]};
        const double b[3] = {v[6], v[7], v[8]};
        const double energy = 0.5 * v[9];
        double tw[3] = {prev[0], prev[1], prev[2]};
        double ts[3] = {0.0, 0.0, 0.0};
        bool finite = true;
        for (int i = 0; i < 9; ++i) finite = finite && isfinite(a[i]);
        double inv[9];
        const int skipped = finite && invert3(a, inv) ? 0 : 1;
        if (skipped == 0) {
            for (int i = 0; i < 3; ++i) ts[i] = (inv[i * 3] * b[0] + inv[i * 3 + 1] * b[1]) + inv[i * 3 + 2] * b[2];
            for (int i = 0; i < 3; ++i) tw[i] = tw[i] + p.rate * (ts[i] - tw[i]);
        }
        for (int i = 0; i < 3; ++i) tw_out[i] = tw[i];
        if (blockIdx.x == 0) {
            double* r = records + (size_t)(k - 1) * kRec;
            for (int i = 0; i < 3; ++i) { r[i] = ts[i]; r[3 + i] = tw[i]; r[16 + i] = b[i]; }
            r[6] = energy;
            for (int i = 0; i < 9; ++i) r[7 + i] = a[i];
            r[19] = (double)skipped;
            for (int i = 20; i < kRec; ++i) r[i] = 0.0;
            if (twist_final)
                for (int i = 0; i < 3; ++i) twist_final[i] = tw[i];
        }
    }
    __syncthreads();
}

// the pose of one launch from the twist: twist_vector_to_matrix2d(-twist) rows 0 and 1 (m) and, for the live field,
// twist_vector_to_matrix3d([t0, 0, t1, 0, t2, 0]) of the float32-rounded twist rows 0..2 (e): cv2.Rodrigues evaluates in
// float64 and rounds to the input's float32
__device__ inline void make_pose(const double* tw, double* m, double* e) {
    const double th = -tw[2];
    const double c2 = cos(th), s2 = sin(th);
    m[0] = c2; m[1] = -s2; m[2] = -tw[0];
    m[3] = s2; m[4] = c2; m[5] = -tw[1];
    const double r[3] = {0.0, (double)(float)tw[2], 0.0};
    const double theta = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    double rot[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (!(theta < 2.220446049250313e-16)) {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
        const double u[3] = {r[0] * itheta, r[1] * itheta, r[2] * itheta};
        const double rx[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                rot[i * 3 + j] = (c * (i == j ? 1.0 : 0.0) + c1 * (u[i] * u[j])) + s * rx[i * 3 + j];
    }
    const double t[3] = {(double)(float)tw[0], 0.0, (double)(float)tw[1]};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) e[i * 4 + j] = (double)(float)rot[i * 3 + j];
        e[i * 4 + 3] = t[i];
    }
}

template <int MODE, typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void rigid_kernel(const float* __restrict__ live_in,
                                                       const float* __restrict__ canonical,
                                                       const DT* __restrict__ depth, float* __restrict__ gradient_out,
                                                       double* __restrict__ twist_io, double* __restrict__ records,
                                                       double* __restrict__ scratch, RigidDev p, int k) {
    __shared__ float tile[kRH][kRH + 1];
    __shared__ double red[kBlock / kWave][kSums];
    __shared__ double tw[3], m[6], e[12];

    if (MODE == GRADIENT) {
        if (threadIdx.x == 0)
            for (int i = 0; i < 3; ++i) tw[i] = p.twist[i];
    } else if (k == 0) {
        if (threadIdx.x == 0)
            for (int i = 0; i < 3; ++i) tw[i] = twist_io[i];
    } else {
        // the twist before iteration k-1: record k-2's, or the initial one.  The finishing launch has one block, which
        // reads twist_io before it writes it.
        const double* prev = k >= 2 ? records + (size_t)(k - 2) * kRec + 3 : twist_io;
        combine_and_update(p, k, prev, records, scratch, red, tw, MODE == FINISH ? twist_io : nullptr);
    }
    if (MODE == FINISH) return;
    if (threadIdx.x == 0) make_pose(tw, m, e);
    __syncthreads();

    double acc[kSums];
#pragma unroll
    for (int c = 0; c < kSums; ++c) acc[c] = 0.0;
    const int ly = threadIdx.x / kRT, lx = threadIdx.x % kRT;
    const float neg_eta = -p.eta;
    for (int ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) {
        const int x0 = (ti % p.tiles_x) * kRT, y0 = (ti / p.tiles_x) * kRT;
        for (int i = threadIdx.x; i < kRH * kRH; i += kBlock) {
            const int hy = i / kRH, hx = i % kRH;
            const int gy = y0 + hy - 1, gx = x0 + hx - 1;
            if (gy >= 0 && gy < p.h && gx >= 0 && gx < p.w) {
                float v;
                if (MODE == GRADIENT) v = live_in[gy * p.w + gx];
                else v = typed_tsdf_voxel<2, double, PT, DT>(depth, p.t, e, gx, gy, 0);
                tile[hy][hx] = v;
            }
        }
        __syncthreads();
        const int y = y0 + ly, x = x0 + lx;
        if (y < p.h && x < p.w) {
            const float l = tile[ly + 1][lx + 1];
            // np.gradient: second-order central differences inside, first-order one-sided at the edges
            const float gy = y == 0 ? tile[ly + 2][lx + 1] - l
                           : (y == p.h - 1 ? l - tile[ly][lx + 1] : (tile[ly + 2][lx + 1] - tile[ly][lx + 1]) / 2.0f);
            const float gx = x == 0 ? tile[ly + 1][lx + 2] - l
                           : (x == p.w - 1 ? l - tile[ly + 1][lx] : (tile[ly + 1][lx + 2] - tile[ly + 1][lx]) / 2.0f);
            const float xv = (float)(((double)x + p.t.off[0]) * p.voxel_size);
            const float zv = (float)(((double)y + p.t.off[2]) * p.voxel_size);
            const double trans0 = (m[0] * (double)xv + m[1] * (double)zv) + m[2] * 1.0;
            const double trans1 = (m[3] * (double)xv + m[4] * (double)zv) + m[5] * 1.0;
            const double fx = (double)gx, fy = (double)gy;
            const float g0 = (float)(fx * 1.0 + fy * 0.0) / p.voxel_size_f;
            const float g1 = (float)(fx * 0.0 + fy * 1.0) / p.voxel_size_f;
            const float g2 = (float)(fx * trans1 + fy * -trans0) / p.voxel_size_f;
            if (MODE == GRADIENT) {
                float* o = gradient_out + ((size_t)y * p.w + x) * 3;
                o[0] = g0; o[1] = g1; o[2] = g2;
            } else {
                const float c = canonical[y * p.w + x];
                acc[0] += (double)(g0 * g0);
                acc[1] += (double)(g0 * g1);
                acc[2] += (double)(g0 * g2);
                acc[3] += (double)(g1 * g1);
                acc[4] += (double)(g1 * g2);
                acc[5] += (double)(g2 * g2);
                const double r = (double)(c - l) + (((double)g0 * tw[0] + (double)g1 * tw[1]) + (double)g2 * tw[2]);
                acc[6] += r * (double)g0;
                acc[7] += r * (double)g1;
                acc[8] += r * (double)g2;
                const double d = (double)c * (c > neg_eta ? 1.0 : 0.0) - (double)l * (l > neg_eta ? 1.0 : 0.0);
                acc[9] += d * d;
            }
        }
        __syncthreads();
    }
    if (MODE == ITERATE) {
        block_sum(acc, red);
        if (threadIdx.x == 0) {
            double* part = scratch + (size_t)(k & 1) * kMaxBlocks * kSums + (size_t)blockIdx.x * kSums;
#pragma unroll
            for (int c = 0; c < kSums; ++c) part[c] = acc[c];
        }
    }
}

int convert(const lsf_rigid_params* params, RigidDev& p) {
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_tsdf_params& t = params->tsdf;
    if (params->height < 2 || params->width < 2 || (long long)params->height * params->width > 0x7fffffffll)
        return LSF_ERR_BAD_ARGUMENT;
    if (!(params->voxel_size > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    p.t.fx = t.intrinsics[0]; p.t.fy = t.intrinsics[1]; p.t.cx = t.intrinsics[2]; p.t.cy = t.intrinsics[3];
    p.t.depth_unit_ratio = t.depth_unit_ratio;
    p.t.voxel_size = t.voxel_size;
    p.t.half_width = t.narrow_band_half_width;
    for (int i = 0; i < 3; ++i) { p.t.off[i] = params->array_offset[i]; p.twist[i] = params->twist[i]; }
    p.t.width = t.image_width; p.t.height = t.image_height; p.t.image_y = t.image_y_coordinate;
    p.t.default_value = t.default_value;
    p.rate = params->rate;
    p.eta = params->eta;
    p.voxel_size = params->voxel_size;
    p.voxel_size_f = (float)params->voxel_size;
    p.h = params->height; p.w = params->width;
    p.tiles_x = (p.w + kRT - 1) / kRT;
    p.tiles = p.tiles_x * ((p.h + kRT - 1) / kRT);
    p.nblocks = p.tiles < kMaxBlocks ? p.tiles : kMaxBlocks;
    return 0;
}

template <typename DT, typename PT>
int launch_run(const float* canonical, const void* live_depth, double* twist, double* records, double* scratch,
               const RigidDev& p, int iterations, hipStream_t s) {
    const DT* d = reinterpret_cast<const DT*>(live_depth);
    for (int k = 0; k < iterations; ++k) {
        hipLaunchKernelGGL((rigid_kernel<ITERATE, DT, PT>), dim3(p.nblocks), dim3(kBlock), 0, s, nullptr, canonical, d,
                           nullptr, twist, records, scratch, p, k);
        if (int e = launch_status()) return e;
    }
    hipLaunchKernelGGL((rigid_kernel<FINISH, DT, PT>), dim3(1), dim3(kBlock), 0, s, nullptr, canonical, d, nullptr,
                       twist, records, scratch, p, iterations);
    return launch_status();
}

template <typename PT>
int launch_run_depth(int32_t depth_dtype, const float* canonical, const void* live_depth, double* twist,
                     double* records, double* scratch, const RigidDev& p, int iterations, hipStream_t s) {
    if (depth_dtype == LSF_DEPTH_U16)
        return launch_run<unsigned short, PT>(canonical, live_depth, twist, records, scratch, p, iterations, s);
    if (depth_dtype == LSF_DEPTH_F32)
        return launch_run<float, PT>(canonical, live_depth, twist, records, scratch, p, iterations, s);
    return launch_run<double, PT>(canonical, live_depth, twist, records, scratch, p, iterations, s);
}

}  // namespace

extern "C" int lsf_rigid_gradient(const float* live, float* gradient_out, const lsf_rigid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live || !gradient_out) return LSF_ERR_BAD_ARGUMENT;
    RigidDev p;
    if (int e = convert(params, p)) return e;
    hipLaunchKernelGGL((rigid_kernel<GRADIENT, float, double>), dim3(p.tiles), dim3(kBlock), 0, as_stream(stream), live,
                       nullptr, nullptr, gradient_out, nullptr, nullptr, nullptr, p, 0);
    return launch_status();
}

extern "C" int lsf_rigid_run(const float* canonical, const void* live_depth, double* twist_inout, double* records,
                             void* scratch, const lsf_rigid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!canonical || !live_depth || !twist_inout || !scratch || !params) return LSF_ERR_BAD_ARGUMENT;
    RigidDev p;
    if (int e = convert(params, p)) return e;
    const lsf_tsdf_params& t = params->tsdf;
    const int it = params->iterations;
    if (it < 0 || (it > 0 && !records)) return LSF_ERR_BAD_ARGUMENT;
    if (t.image_width <= 0 || t.image_height <= 0 || !(t.narrow_band_half_width > 0.0) || t.image_y_coordinate < 0 ||
        t.image_y_coordinate >= t.image_height)
        return LSF_ERR_BAD_ARGUMENT;
    const int dt = params->depth_dtype;
    if (dt != LSF_DEPTH_U16 && dt != LSF_DEPTH_F32 && dt != LSF_DEPTH_F64) return LSF_ERR_BAD_ARGUMENT;
    if (it == 0) return 0;
    double* sc = reinterpret_cast<double*>(scratch);
    hipStream_t s = as_stream(stream);
    if (t.intrinsics_are_f32) return launch_run_depth<float>(dt, canonical, live_depth, twist_inout, records, sc, p, it, s);
    return launch_run_depth<double>(dt, canonical, live_depth, twist_inout, records, sc, p, it, s);
}
