// SDF-2-SDF rigid 3-D tracker, 6-DoF (include/lsf_hip.h, lsf_rigid3d_*): the reference's 2-D algorithm
// (rigid_opt/sdf_2_sdf_optimizer2d.py:60-137, rigid_opt/sdf_gradient_field.py:13-38) lifted to a volume, with the dtypes
// of lsf_rigid.hip.  One kernel, three modes, as the 2-D one (RigidMode, lsf_rigid_solve.h):
//   GRADIENT  the twist gradient of a given live volume, or of the live volume generated under a given twist (one launch)
//   ITERATE   iteration k of optimize(): prologue = rigid_prologue<6> (combine iteration k-1's per-block partial sums,
//             singular test, 6x6 solve and update -- every block computes the same twist bit for bit, block 0 writes
//             record k-1); body = march a 16 x 16 x-y tile plus a one-voxel halo along z through a ring of planes in
//             LDS, generating one new live plane per step under the pose, np.gradient, twist gradient, and the 28
//             float64 sums of A, b and the energy kept in registers; one wave / block reduction at the end into this
//             block's partial (ping-pong buffer k & 1)
//   FINISH    the prologue alone for the last iteration, one block; writes the final twist
// Per-voxel arithmetic is bit-identical to tests/rigid3d_restatement.py under -ffp-contract=off; the sums are tree
// reductions.
#include "lsf_device.h"
#include "lsf_rigid_solve.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kRT = 16;          // tile edge: 16 x 16 voxels = one thread each
constexpr int kRH = kRT + 2;     // with the one-voxel halo
constexpr int kSlots = 4;        // ring of live planes: z - 1, z, z + 1 and the one being generated
constexpr int kSums = RigidLayout<6>::kSums;  // A's upper triangle (21, row by row), b (6), energy
constexpr int kMaxBlocks = RigidLayout<6>::kMaxBlocks;
constexpr int kMinChunk = 4;     // the shortest z run of one work item (2 halo planes per run)
static_assert(kBlock == kRT * kRT, "one thread per tile voxel");
static_assert(kRH * kRH <= 2 * kBlock, "a plane with its halo is generated in two passes");

struct Rigid3dDev {
    TypedTsdf t;
    double voxel_size;  // the gradient's voxel size (t.voxel_size is the generator's)
    double twist[6];    // GRADIENT
    double rate;
    float eta;
    float voxel_size_f;
    int nz, ny, nx;
    int tiles_x, tiles_xy;  // x-y tiles
    int zc;                 // z extent of one work item
    int items;              // tiles_xy * ceil(nz / zc): (tile, z-chunk) pairs, item = chunk * tiles_xy + tile
    int nblocks;            // the grid: min(items, kMaxBlocks), the number of partials
};

// the pose of one launch from the twist, rows 0..2 row-major: m = twist_vector_to_matrix3d(-twist) in float64 (the
// gradient's p), e = the live volume's extrinsic (live_extrinsic, lsf_tsdf_typed.h)
__device__ inline void make_pose(const double* tw, double* m, double* e) {
    double r[3], rot[9];
    live_extrinsic(tw, e);
    for (int i = 0; i < 3; ++i) r[i] = -tw[3 + i];
    rodrigues(r, rot);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[i * 4 + j] = rot[i * 3 + j];
        m[i * 4 + 3] = -tw[i];
    }
}

template <int MODE, typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void rigid3d_kernel(const float* __restrict__ live_in,
                                                         const float* __restrict__ canonical,
                                                         const DT* __restrict__ depth, float* __restrict__ live_out,
                                                         float* __restrict__ gradient_out, double* __restrict__ twist_io,
                                                         double* __restrict__ records, double* __restrict__ scratch,
                                                         Rigid3dDev p, int k) {
    __shared__ float ring[kSlots][kRH][kRH + 1];
    __shared__ double red[kBlock / kWave][kSums];
    __shared__ double tw[6], m[12], e[12];

    rigid_prologue<MODE, 6>(p, k, twist_io, records, scratch, red, tw);
    if (MODE == FINISH) return;
    if (threadIdx.x == 0) make_pose(tw, m, e);
    __syncthreads();

    double acc[kSums];
#pragma unroll
    for (int c = 0; c < kSums; ++c) acc[c] = 0.0;
    const int ly = threadIdx.x / kRT, lx = threadIdx.x % kRT;
    const float neg_eta = -p.eta;
    const size_t plane = (size_t)p.ny * p.nx;
    for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
        const int tile = item % p.tiles_xy;
        const int x0 = (tile % p.tiles_x) * kRT, y0 = (tile / p.tiles_x) * kRT;
        const int z0 = (item / p.tiles_xy) * p.zc;
        const int z1 = min(z0 + p.zc, p.nz);
        // plane z of the tile and its halo into ring slot z & 3: read, or generated under the pose
        auto fill = [&](int z) {
            for (int i = threadIdx.x; i < kRH * kRH; i += kBlock) {
                const int hy = i / kRH, hx = i % kRH;
                const int gy = y0 + hy - 1, gx = x0 + hx - 1;
                if (gy >= 0 && gy < p.ny && gx >= 0 && gx < p.nx) {
                    float v;
                    if (MODE == GRADIENT && live_in) v = live_in[z * plane + (size_t)gy * p.nx + gx];
                    else v = typed_tsdf_voxel<3, double, PT, DT>(depth, p.t, e, gx, gy, z);
                    ring[z & 3][hy][hx] = v;
                }
            }
        };
        if (z0 > 0) fill(z0 - 1);
        fill(z0);
        const int y = y0 + ly, x = x0 + lx;
        const bool inside = y < p.ny && x < p.nx;
        const float yv = (float)(((double)y + p.t.off[1]) * p.voxel_size);
        const float xv = (float)(((double)x + p.t.off[0]) * p.voxel_size);
        for (int z = z0; z < z1; ++z) {
            // slot (z + 1) & 3 last held z - 3, read by step z - 2, which ended before step z - 1's barrier
            if (z + 1 < p.nz) fill(z + 1);
            __syncthreads();
            if (inside) {
                const float(*s)[kRH + 1] = ring[z & 3];
                const float l = s[ly + 1][lx + 1];
                // np.gradient: second-order central differences inside, first-order one-sided at the faces
                const float gx = x == 0 ? s[ly + 1][lx + 2] - l
                               : (x == p.nx - 1 ? l - s[ly + 1][lx] : (s[ly + 1][lx + 2] - s[ly + 1][lx]) / 2.0f);
                const float gy = y == 0 ? s[ly + 2][lx + 1] - l
                               : (y == p.ny - 1 ? l - s[ly][lx + 1] : (s[ly + 2][lx + 1] - s[ly][lx + 1]) / 2.0f);
                const float gz = z == 0 ? ring[(z + 1) & 3][ly + 1][lx + 1] - l
                               : (z == p.nz - 1 ? l - ring[(z - 1) & 3][ly + 1][lx + 1]
                                                : (ring[(z + 1) & 3][ly + 1][lx + 1] - ring[(z - 1) & 3][ly + 1][lx + 1]) / 2.0f);
                const float zv = (float)(((double)z + p.t.off[2]) * p.voxel_size);
                const double px = ((m[0] * (double)xv + m[1] * (double)yv) + m[2] * (double)zv) + m[3] * 1.0;
                const double py = ((m[4] * (double)xv + m[5] * (double)yv) + m[6] * (double)zv) + m[7] * 1.0;
                const double pz = ((m[8] * (double)xv + m[9] * (double)yv) + m[10] * (double)zv) + m[11] * 1.0;
                const double fx = (double)gx, fy = (double)gy, fz = (double)gz;
                float g[6];
                g[0] = (float)fx / p.voxel_size_f;
                g[1] = (float)fy / p.voxel_size_f;
                g[2] = (float)fz / p.voxel_size_f;
                g[3] = (float)(py * fz - pz * fy) / p.voxel_size_f;
                g[4] = (float)(pz * fx - px * fz) / p.voxel_size_f;
                g[5] = (float)(px * fy - py * fx) / p.voxel_size_f;
                const size_t at = z * plane + (size_t)y * p.nx + x;
                if (MODE == GRADIENT) {
                    if (live_out) live_out[at] = l;
                    if (gradient_out)
#pragma unroll
                        for (int c = 0; c < 6; ++c) gradient_out[at * 6 + c] = g[c];
                } else {
                    const float c = canonical[at];
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = i; j < 6; ++j) acc[q++] += (double)(g[i] * g[j]);
                    double dot = (double)g[0] * tw[0];
#pragma unroll
                    for (int i = 1; i < 6; ++i) dot = dot + (double)g[i] * tw[i];
                    const double r = (double)(c - l) + dot;
#pragma unroll
                    for (int i = 0; i < 6; ++i) acc[21 + i] += r * (double)g[i];
                    const double d = (double)c * (c > neg_eta ? 1.0 : 0.0) - (double)l * (l > neg_eta ? 1.0 : 0.0);
                    acc[27] += d * d;
                }
            }
        }
        __syncthreads();  // the next item's first planes overwrite slots this item's last steps read
    }
    if (MODE == ITERATE) rigid_store_partial<6>(acc, red, scratch, k);
}

int convert(const lsf_rigid3d_params* params, Rigid3dDev& p) {
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_tsdf_params& t = params->tsdf;
    if (params->depth < 2 || params->height < 2 || params->width < 2 ||
        (long long)params->depth * params->height * params->width > 0x7fffffffll)
        return LSF_ERR_BAD_ARGUMENT;
    if (!(params->voxel_size > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    p.t = typed_tsdf(t, params->array_offset, 0);
    for (int i = 0; i < 6; ++i) p.twist[i] = params->twist[i];
    p.rate = params->rate;
    p.eta = params->eta;
    p.voxel_size = params->voxel_size;
    p.voxel_size_f = (float)params->voxel_size;
    p.nz = params->depth; p.ny = params->height; p.nx = params->width;
    p.tiles_x = (p.nx + kRT - 1) / kRT;
    p.tiles_xy = p.tiles_x * ((p.ny + kRT - 1) / kRT);
    // z runs long enough that (tile, run) pairs about fill kMaxBlocks workgroups, and no shorter than kMinChunk
    const long long want = ((long long)p.nz * p.tiles_xy + kMaxBlocks - 1) / kMaxBlocks;
    p.zc = (int)(want < kMinChunk ? kMinChunk : (want > p.nz ? p.nz : want));
    if (p.zc > p.nz) p.zc = p.nz;
    const long long items = (long long)p.tiles_xy * ((p.nz + p.zc - 1) / p.zc);
    p.items = (int)items;
    p.nblocks = items < kMaxBlocks ? (int)items : kMaxBlocks;
    return 0;
}

template <int MODE, typename DT, typename PT>
int launch(const Rigid3dDev& p, unsigned blocks, const float* live, const float* canonical, const void* depth,
           float* live_out, float* gradient_out, double* twist, double* records, double* scratch, int k,
           hipStream_t s) {
    hipLaunchKernelGGL((rigid3d_kernel<MODE, DT, PT>), dim3(blocks), dim3(kBlock), 0, s, live, canonical,
                       reinterpret_cast<const DT*>(depth), live_out, gradient_out, twist, records, scratch, p, k);
    return launch_status();
}

template <typename DT, typename PT>
int launch_run(const float* canonical, const void* live_depth, double* twist, double* records, double* scratch,
               const Rigid3dDev& p, int iterations, hipStream_t s) {
    for (int k = 0; k < iterations; ++k)
        if (int e = launch<ITERATE, DT, PT>(p, p.nblocks, nullptr, canonical, live_depth, nullptr, nullptr, twist,
                                            records, scratch, k, s))
            return e;
    return launch<FINISH, DT, PT>(p, 1, nullptr, canonical, live_depth, nullptr, nullptr, twist, records, scratch,
                                  iterations, s);
}

}  // namespace

extern "C" int lsf_rigid3d_gradient(const float* live, const void* live_depth, float* live_out, float* gradient_out,
                                    const lsf_rigid3d_params* params, void* stream) {
    (void)hipGetLastError();
    if ((!live && !live_depth) || (!live_out && !gradient_out)) return LSF_ERR_BAD_ARGUMENT;
    Rigid3dDev p;
    if (int e = convert(params, p)) return e;
    hipStream_t s = as_stream(stream);
    if (live)
        return launch<GRADIENT, float, double>(p, p.nblocks, live, nullptr, nullptr, live_out, gradient_out, nullptr,
                                               nullptr, nullptr, 0, s);
    if (!depth_dtype_ok(params->depth_dtype) || !typed_tsdf_ok(params->tsdf, false, true))
        return LSF_ERR_BAD_ARGUMENT;
    return dispatch_typed(params->depth_dtype, params->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch<GRADIENT, decltype(dt), decltype(pt)>(
            p, p.nblocks, nullptr, nullptr, live_depth, live_out, gradient_out, nullptr, nullptr, nullptr, 0, s);
    });
}

extern "C" int lsf_rigid3d_run(const float* canonical, const void* live_depth, double* twist_inout, double* records,
                               void* scratch, const lsf_rigid3d_params* params, void* stream) {
    (void)hipGetLastError();
    if (!canonical || !live_depth || !twist_inout || !scratch || !params) return LSF_ERR_BAD_ARGUMENT;
    Rigid3dDev p;
    if (int e = convert(params, p)) return e;
    const int it = params->iterations;
    if (it < 0 || (it > 0 && !records)) return LSF_ERR_BAD_ARGUMENT;
    if (!depth_dtype_ok(params->depth_dtype) || !typed_tsdf_ok(params->tsdf, false, true))
        return LSF_ERR_BAD_ARGUMENT;
    if (it == 0) return 0;
    double* sc = reinterpret_cast<double*>(scratch);
    hipStream_t s = as_stream(stream);
    return dispatch_typed(params->depth_dtype, params->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch_run<decltype(dt), decltype(pt)>(canonical, live_depth, twist_inout, records, sc, p, it, s);
    });
}
