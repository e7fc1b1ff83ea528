// SDF-2-SDF rigid 2-D tracker (reference rigid_opt/sdf_2_sdf_optimizer2d.py:60-137, rigid_opt/sdf_gradient_field.py:
// 13-38, math_utils/transformation.py:11-34).  One kernel, three modes (RigidMode, lsf_rigid_solve.h):
//   GRADIENT  calculate_gradient_wrt_twist of a given live field and twist (one launch)
//   ITERATE   iteration k of optimize(): prologue = rigid_prologue<3> (combine iteration k-1's per-block partial sums,
//             singular test, 3x3 solve and update -- every block computes the same twist bit for bit, block 0 writes
//             record k-1); body = regenerate the live TSDF of a 16 x 16 tile plus a one-voxel halo in LDS under the
//             pose, np.gradient, twist gradient, and the 10 float64 sums of A, b and the energy, reduced through the
//             wave and the block into this block's partial (ping-pong buffer k & 1)
//   FINISH    the prologue alone for the last iteration, one block; writes the final twist
// Per-voxel arithmetic follows the reference's dtypes (tests/rigid_restatement.py) and is bit-identical to the
// restatement under -ffp-contract=off; the sums are tree reductions, not the reference's sequential loop.
#include "lsf_device.h"
#include "lsf_rigid_solve.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kRT = 16;          // tile edge: 16 x 16 voxels = one thread each
constexpr int kRH = kRT + 2;     // with the one-voxel halo
constexpr int kSums = RigidLayout<3>::kSums;  // A (6: 00 01 02 11 12 22), b (3), energy
constexpr int kMaxBlocks = RigidLayout<3>::kMaxBlocks;
static_assert(kBlock == kRT * kRT, "one thread per tile voxel");

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

// the pose of one launch from the twist: twist_vector_to_matrix2d(-twist) rows 0 and 1 (m) and, for the live field,
// the live extrinsic of the 6-DoF twist [t0, 0, t1, 0, t2, 0] (e, lsf_tsdf_typed.h)
__device__ inline void make_pose(const double* tw, double* m, double* e) {
    const double th = -tw[2];
    const double c2 = cos(th), s2 = sin(th);
    m[0] = c2; m[1] = -s2; m[2] = -tw[0];
    m[3] = s2; m[4] = c2; m[5] = -tw[1];
    const double tw6[6] = {tw[0], 0.0, tw[1], 0.0, tw[2], 0.0};
    live_extrinsic(tw6, e);
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

    rigid_prologue<MODE, 3>(p, k, twist_io, records, scratch, red, tw);
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
    if (MODE == ITERATE) rigid_store_partial<3>(acc, red, scratch, k);
}

int convert(const lsf_rigid_params* params, RigidDev& p) {
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_tsdf_params& t = params->tsdf;
    if (params->height < 2 || params->width < 2 || (long long)params->height * params->width > 0x7fffffffll)
        return LSF_ERR_BAD_ARGUMENT;
    if (!(params->voxel_size > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    p.t = typed_tsdf(t, params->array_offset, t.image_y_coordinate);
    for (int i = 0; i < 3; ++i) p.twist[i] = params->twist[i];
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
    // the depth row must be in the image; width x height is not bounded here (lsf_rigid3d_* bound it)
    if (!typed_tsdf_ok(t, true, false) || !depth_dtype_ok(params->depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    if (it == 0) return 0;
    double* sc = reinterpret_cast<double*>(scratch);
    hipStream_t s = as_stream(stream);
    return dispatch_typed(params->depth_dtype, t.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch_run<decltype(dt), decltype(pt)>(canonical, live_depth, twist_inout, records, sc, p, it, s);
    });
}
