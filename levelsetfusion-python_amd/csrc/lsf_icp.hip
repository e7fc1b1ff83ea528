// Projective point-to-plane ICP against the ray-cast prediction (include/lsf_hip.h, lsf_icp_run): the KinectFusion
// tracker, which the reference does not have.  The arithmetic is INTEGRATION.md section 3 ("Projective ICP");
// tests/icp_restatement.py restates it.  Every per-pixel step is one float64 operation in the order written there;
// -ffp-contract=off keeps products and sums separately rounded, so the residual image and the correspondence count
// equal the restatement bit for bit.  One kernel, two modes, with the 3-D rigid tracker's schedule (RigidMode,
// lsf_rigid_solve.h):
//   ITERATE  iteration k: prologue = combine iteration k-1's per-block partial sums in a fixed order, solve the 6 x 6
//            system, compose the step into the twist (every block computes the same twist bit for bit, block 0 writes
//            record k-1); body = one lane per strided live pixel, a wave per 8 x 8 block of them, a grid-stride loop
//            over 16 x 16 tiles, the 29 float64 sums kept in registers; one block reduction at the end into this
//            block's partial (ping-pong buffer k & 1)
//   FINISH   the prologue alone for the last iteration, one block; writes the final twist
// The partials cross launch boundaries only: no float atomics, no in-launch hand-off, so a rerun is bit-identical.
// lsf_icp_run_pyramid is the same schedule over a live depth pyramid (lsf_depth_pyramid's output): a lane per pixel
// of the level, back-projected with the level's intrinsics, an optional normal-angle gate after the distance test, and
// a 30th sum, the pairs the gate rejected (record slot 58).
#include "lsf_device.h"
#include "lsf_rigid_solve.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kTile = 16;  // a workgroup covers 16 x 16 strided pixels
constexpr int kSub = 8;    // a wave's block is kSub x kSub of them
constexpr int kSums = 29;  // A's upper triangle (21, row by row), b (6), energy, count
constexpr int kPyrSums = 30;  // lsf_icp_run_pyramid: and the pairs the angle gate rejected
constexpr int kMaxBlocks = LSF_ICP_MAX_BLOCKS;
constexpr int kRecord = LSF_ICP_RECORD_DOUBLES;
constexpr int kDelta = 0, kTwist = 6, kEnergy = 12, kA = 13, kB = 49, kSkipped = 55, kCount = 56, kLevel = 57,
              kRejected = 58;
static_assert(kSub * kSub == kWave && (kTile / kSub) * (kTile / kSub) * kWave == kBlock, "4 waves of 8 x 8 pixels");
static_assert(LSF_ICP_SCRATCH_BYTES == 2 * kMaxBlocks * kSums * 8, "two ping-pong buffers of kMaxBlocks partials");
static_assert(LSF_ICP_PYRAMID_SCRATCH_BYTES == 2 * kMaxBlocks * kPyrSums * 8, "the same with the 30th sum");
static_assert(kMaxBlocks <= kBlock, "the prologue gives every partial one thread");
static_assert(kRejected < kRecord && kB == kA + 36 && kSkipped == kB + 6, "the record holds every field");

struct IcpDev {
    double fx, fy, cx, cy, ratio, max_distance;
    double twist_p[6];  // the prediction's camera: live_extrinsic(twist_p), the ray-cast's
    int height, width;
};

// the strided pixel grid of one launch's level
struct Level {
    int stride, ni, nj;  // pixels (stride i, stride j), i < ni, j < nj
    int tiles_x, tiles;  // 16 x 16 tiles of the strided grid
};

// one level of the live pyramid: every pixel (i, j), i < ni, j < nj, at offset + j ni, back-projected with fx ... cy
struct PyrLevel {
    double fx, fy, cx, cy;
    long long offset;
    int ni, nj;
    int tiles_x, tiles;
};

// the twist after the step delta = (tau, omega): R' = R Rodrigues(omega)^T, t' = t - R' tau, out = (t', log R')
__device__ inline void compose(const double* tw, const double* delta, double* out) {
    double R[9], D[9], Rn[9];
    rodrigues(tw + 3, R);
    rodrigues(delta + 3, D);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (R[i * 3] * D[j * 3] + R[i * 3 + 1] * D[j * 3 + 1]) + R[i * 3 + 2] * D[j * 3 + 2];
    for (int i = 0; i < 3; ++i)
        out[i] = tw[i] - ((Rn[i * 3] * delta[0] + Rn[i * 3 + 1] * delta[1]) + Rn[i * 3 + 2] * delta[2]);
    // log: theta = atan2(|w|, (tr R' - 1) / 2), w = vee(R' - R'^T) / 2; accurate away from theta = pi only
    const double w[3] = {(Rn[7] - Rn[5]) / 2.0, (Rn[2] - Rn[6]) / 2.0, (Rn[3] - Rn[1]) / 2.0};
    const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    if (nw == 0.0) {
        for (int i = 0; i < 3; ++i) out[3 + i] = 0.0;
        return;
    }
    const double tr = (Rn[0] + Rn[4]) + Rn[8];
    const double s = atan2(nw, (tr - 1.0) / 2.0) / nw;
    for (int i = 0; i < 3; ++i) out[3 + i] = w[i] * s;
}

// the twist of launch k into tw (LDS): twist_io (k = 0), or iteration k-1's partials (prev_blocks of them) combined,
// solved and composed onto the twist before it (record k-2's, or twist_io); block 0 writes record k-1 and, with
// twist_final, the final twist.  The finishing launch has one block, which reads twist_io before it writes it.
// K = kPyrSums also writes the gate's rejections to record slot kRejected.
template <int K>
__device__ __forceinline__ void icp_prologue(int k, int prev_blocks, int prev_level, double* __restrict__ twist_io,
                                             double* __restrict__ records, const double* __restrict__ scratch,
                                             double (*red)[K], double* tw, double* twist_final) {
    if (k == 0) {
        if (threadIdx.x == 0)
            for (int i = 0; i < 6; ++i) tw[i] = twist_io[i];
        __syncthreads();
        return;
    }
    double v[K];
    combine_partials(scratch + (size_t)((k - 1) & 1) * kMaxBlocks * K, prev_blocks, v, red);
    if (threadIdx.x == 0) {
        const double* prev = k >= 2 ? records + (size_t)(k - 2) * kRecord + kTwist : twist_io;
        double a[36], b[6], delta[6], next[6];
        normal_equations<6>(v, a, b);
        for (int i = 0; i < 6; ++i) { delta[i] = 0.0; next[i] = prev[i]; }
        const int skipped = solve<6>(a, b, delta);
        if (skipped == 0) compose(prev, delta, next);
        for (int i = 0; i < 6; ++i) tw[i] = next[i];
        if (blockIdx.x == 0) {
            double* r = records + (size_t)(k - 1) * kRecord;
            for (int i = 0; i < 6; ++i) { r[kDelta + i] = delta[i]; r[kTwist + i] = next[i]; r[kB + i] = b[i]; }
            r[kEnergy] = v[27];
            for (int i = 0; i < 36; ++i) r[kA + i] = a[i];
            r[kSkipped] = (double)skipped;
            r[kCount] = v[28];
            r[kLevel] = (double)prev_level;
            int i = kLevel + 1;
            if constexpr (K == kPyrSums) r[i++] = v[kSums];
            for (; i < kRecord; ++i) r[i] = 0.0;
            if (twist_final)
                for (int i = 0; i < 6; ++i) twist_final[i] = next[i];
        }
    }
    __syncthreads();
}

// the poses of launch k into e (the estimate, from the unrounded float64 twist tw) and ep (the prediction's camera),
// via LDS; every thread of the block calls it
__device__ __forceinline__ void load_poses(const double* tw, const IcpDev& p, double* pose, double* pose_p,
                                           double (&e)[12], double (&ep)[12]) {
    if (threadIdx.x == 0) {
        double R[9];
        rodrigues(tw + 3, R);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) pose[i * 4 + j] = R[i * 3 + j];
            pose[i * 4 + 3] = tw[i];
        }
        live_extrinsic(p.twist_p, pose_p);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 12; ++q) { e[q] = pose[q]; ep[q] = pose_p[q]; }
}

// the live vertex vx (camera coordinates) against the prediction at the estimate e: its residual r, the pair's terms
// added to acc, when the pair is valid and (GATE) the live normal nl passes the angle gate; NaN otherwise.  A pair
// that passes the distance test and fails the gate counts in acc[kSums].
template <bool GATE, int K>
__device__ __forceinline__ float accumulate_pair(const double (&vx)[3], const double (&e)[12], const double (&ep)[12],
                                                 const IcpDev& p, const float* __restrict__ pred_depth,
                                                 const float* __restrict__ pred_normals, const float* __restrict__ nl,
                                                 double cos_max, double (&acc)[K]) {
    double dv[3], g[3], q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dv[c] = vx[c] - e[c * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (e[c] * dv[0] + e[4 + c] * dv[1]) + e[8 + c] * dv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((ep[c * 4] * g[0] + ep[c * 4 + 1] * g[1]) + ep[c * 4 + 2] * g[2]) + ep[c * 4 + 3];
    if (!(q[2] > 0.0)) return NAN;
    const double fu = rint((p.fx * q[0]) / q[2] + p.cx), fv = rint((p.fy * q[1]) / q[2] + p.cy);
    // compared as doubles first: NaN and far-off values never reach the integer conversion
    if (!(fu >= 0.0 && fu <= (double)(p.width - 1) && fv >= 0.0 && fv <= (double)(p.height - 1))) return NAN;
    const long long at = (long long)(int)fv * p.width + (int)fu;
    const double D = (double)pred_depth[at];
    const double n[3] = {(double)pred_normals[at * 3], (double)pred_normals[at * 3 + 1],
                         (double)pred_normals[at * 3 + 2]};
    if (!(D > 0.0 && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0))) return NAN;
    const double V[3] = {D * ((fu - p.cx) / p.fx), D * ((fv - p.cy) / p.fy), D * 1.0};
    double dV[3], Vw[3], Nw[3], diff[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dV[c] = V[c] - ep[c * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Vw[c] = (ep[c] * dV[0] + ep[4 + c] * dV[1]) + ep[8 + c] * dV[2];
        Nw[c] = (ep[c] * n[0] + ep[4 + c] * n[1]) + ep[8 + c] * n[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) diff[c] = g[c] - Vw[c];
    const double dist = sqrt((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]);
    if (!(dist <= p.max_distance)) return NAN;
    if constexpr (GATE) {  // the live normal in world directions, m = R^T n, against N_w
        const double ln[3] = {(double)nl[0], (double)nl[1], (double)nl[2]};
        bool keep = ln[0] != 0.0 || ln[1] != 0.0 || ln[2] != 0.0;
        if (keep) {
            double m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = (e[c] * ln[0] + e[4 + c] * ln[1]) + e[8 + c] * ln[2];
            keep = (m[0] * Nw[0] + m[1] * Nw[1]) + m[2] * Nw[2] >= cos_max;
        }
        if (!keep) {
            acc[kSums] += 1.0;
            return NAN;
        }
    }
    const double r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2];
    const double J[6] = {Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
                         g[0] * Nw[1] - g[1] * Nw[0]};
    int s = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[s++] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] -= J[a] * r;
    acc[27] += r * r;
    acc[28] += 1.0;
    return (float)r;
}

template <int MODE, typename DT>
__global__ __launch_bounds__(kBlock) void icp_kernel(const DT* __restrict__ live, const float* __restrict__ pred_depth,
                                                     const float* __restrict__ pred_normals,
                                                     double* __restrict__ twist_io, double* __restrict__ records,
                                                     double* __restrict__ scratch, float* __restrict__ residuals,
                                                     IcpDev p, Level lv, int k, int prev_blocks, int prev_level) {
    __shared__ double red[kBlock / kWave][kSums];
    __shared__ double tw[6], pose[12], pose_p[12];

    icp_prologue<kSums>(k, prev_blocks, prev_level, twist_io, records, scratch, red, tw,
                        MODE == FINISH ? twist_io : nullptr);
    if (MODE == FINISH) return;
    double e[12], ep[12];
    load_poses(tw, p, pose, pose_p, e, ep);

    double acc[kSums];
#pragma unroll
    for (int c = 0; c < kSums; ++c) acc[c] = 0.0;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ox = (wave % (kTile / kSub)) * kSub + lane % kSub, oy = (wave / (kTile / kSub)) * kSub + lane / kSub;
    for (int tile = blockIdx.x; tile < lv.tiles; tile += gridDim.x) {
        const int i = (tile % lv.tiles_x) * kTile + ox, j = (tile / lv.tiles_x) * kTile + oy;
        if (i >= lv.ni || j >= lv.nj) continue;
        const int u = i * lv.stride, v = j * lv.stride;  // < width, height: ni = ceil(width / stride)
        const double d = (double)scaled_depth(live, (long long)v * p.width + u, p.ratio);
        float res = NAN;
        if (d > 0.0) {  // NaN is not > 0
            const double vx[3] = {d * (((double)u - p.cx) / p.fx), d * (((double)v - p.cy) / p.fy), d * 1.0};
            res = accumulate_pair<false>(vx, e, ep, p, pred_depth, pred_normals, nullptr, 0.0, acc);
        }
        if (residuals) {  // the last iteration: r at the pixel, NaN at the rest of its stride x stride cell
            for (int y = v; y < min(v + lv.stride, p.height); ++y)
                for (int x = u; x < min(u + lv.stride, p.width); ++x)
                    residuals[(long long)y * p.width + x] = (x == u && y == v) ? res : NAN;
        }
    }
    store_partial(acc, red, scratch + (size_t)(k & 1) * kMaxBlocks * kSums);
}

// lsf_icp_run_pyramid: every pixel of the pyramid level lv, float32 metres, its vertex from the level's intrinsics
template <int MODE, bool GATE>
__global__ __launch_bounds__(kBlock) void icp_pyramid_kernel(const float* __restrict__ live,
                                                             const float* __restrict__ live_normals,
                                                             const float* __restrict__ pred_depth,
                                                             const float* __restrict__ pred_normals,
                                                             double* __restrict__ twist_io, double* __restrict__ records,
                                                             double* __restrict__ scratch, float* __restrict__ residuals,
                                                             IcpDev p, PyrLevel lv, double cos_max, int k,
                                                             int prev_blocks, int prev_level) {
    __shared__ double red[kBlock / kWave][kPyrSums];
    __shared__ double tw[6], pose[12], pose_p[12];

    icp_prologue<kPyrSums>(k, prev_blocks, prev_level, twist_io, records, scratch, red, tw,
                           MODE == FINISH ? twist_io : nullptr);
    if (MODE == FINISH) return;
    double e[12], ep[12];
    load_poses(tw, p, pose, pose_p, e, ep);

    double acc[kPyrSums];
#pragma unroll
    for (int c = 0; c < kPyrSums; ++c) acc[c] = 0.0;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ox = (wave % (kTile / kSub)) * kSub + lane % kSub, oy = (wave / (kTile / kSub)) * kSub + lane / kSub;
    for (int tile = blockIdx.x; tile < lv.tiles; tile += gridDim.x) {
        const int i = (tile % lv.tiles_x) * kTile + ox, j = (tile / lv.tiles_x) * kTile + oy;
        if (i >= lv.ni || j >= lv.nj) continue;
        const long long at = (long long)j * lv.ni + i;
        const double d = (double)live[lv.offset + at];
        float res = NAN;
        if (d > 0.0) {
            const double vx[3] = {d * (((double)i - lv.cx) / lv.fx), d * (((double)j - lv.cy) / lv.fy), d * 1.0};
            res = accumulate_pair<GATE>(vx, e, ep, p, pred_depth, pred_normals, live_normals + (lv.offset + at) * 3,
                                        cos_max, acc);
        }
        if (residuals) residuals[at] = res;
    }
    store_partial(acc, red, scratch + (size_t)(k & 1) * kMaxBlocks * kPyrSums);
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

Level level_of(const lsf_icp_params* q, int stride) {
    Level lv;
    lv.stride = stride;
    lv.ni = (q->width + stride - 1) / stride;
    lv.nj = (q->height + stride - 1) / stride;
    lv.tiles_x = (lv.ni + kTile - 1) / kTile;
    lv.tiles = lv.tiles_x * ((lv.nj + kTile - 1) / kTile);
    return lv;
}

template <int MODE, typename DT>
int launch(unsigned blocks, const void* live, const float* pred_depth, const float* pred_normals, double* twist,
           double* records, double* scratch, float* residuals, const IcpDev& p, const Level& lv, int k,
           int prev_blocks, int prev_level, hipStream_t s) {
    hipLaunchKernelGGL((icp_kernel<MODE, DT>), dim3(blocks), dim3(kBlock), 0, s, reinterpret_cast<const DT*>(live),
                       pred_depth, pred_normals, twist, records, scratch, residuals, p, lv, k, prev_blocks,
                       prev_level);
    return launch_status();
}

template <typename DT>
int launch_run(const lsf_icp_params* q, const IcpDev& p, const void* live, const float* pred_depth,
               const float* pred_normals, double* twist, double* records, double* scratch, float* residuals,
               int total, hipStream_t s) {
    int k = 0, prev_blocks = 0, prev_level = 0;
    Level lv = level_of(q, 1);
    for (int l = 0; l < q->levels; ++l) {
        lv = level_of(q, q->strides[l]);
        const int blocks = lv.tiles < kMaxBlocks ? lv.tiles : kMaxBlocks;
        for (int it = 0; it < q->iterations[l]; ++it, ++k) {
            if (int e = launch<ITERATE, DT>(blocks, live, pred_depth, pred_normals, twist, records, scratch,
                                            k == total - 1 ? residuals : nullptr, p, lv, k, prev_blocks, prev_level,
                                            s))
                return e;
            prev_blocks = blocks;
            prev_level = l;
        }
    }
    return launch<FINISH, DT>(1, live, pred_depth, pred_normals, twist, records, scratch, nullptr, p, lv, total,
                              prev_blocks, prev_level, s);
}

}  // namespace

extern "C" int lsf_icp_run(const void* live_depth, const float* pred_depth, const float* pred_normals,
                           double* twist_inout, double* records, void* scratch, float* residuals_out,
                           const lsf_icp_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !pred_depth || !pred_normals || !twist_inout || !scratch || !params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_icp_params* q = params;
    if (q->height < 1 || q->width < 1 || (long long)q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    const double all[] = {q->fx, q->fy, q->cx, q->cy, q->depth_unit_ratio, q->twist_p[0], q->twist_p[1],
                          q->twist_p[2], q->twist_p[3], q->twist_p[4], q->twist_p[5]};
    for (double x : all)
        if (!std::isfinite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->max_distance > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (!depth_dtype_ok(q->depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    if (q->levels < 1 || q->levels > LSF_ICP_MAX_LEVELS) return LSF_ERR_BAD_ARGUMENT;
    long long total = 0;
    for (int l = 0; l < q->levels; ++l) {
        if (q->strides[l] < 1 || q->iterations[l] < 0) return LSF_ERR_BAD_ARGUMENT;
        total += q->iterations[l];
    }
    if (total > 0x7fffffffll / kRecord || (total > 0 && !records)) return LSF_ERR_BAD_ARGUMENT;
    // no output may alias an input or another output
    static const size_t kDepthBytes[3] = {2, 4, 8};
    const size_t pixels = (size_t)q->height * q->width;
    const void* outs[4] = {twist_inout, records, scratch, residuals_out};
    const size_t out_bytes[4] = {6 * 8, (size_t)total * kRecord * 8, LSF_ICP_SCRATCH_BYTES, pixels * 4};
    const void* ins[3] = {live_depth, pred_depth, pred_normals};
    const size_t in_bytes[3] = {pixels * kDepthBytes[q->depth_dtype], pixels * 4, pixels * 12};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j)
            if (overlaps(outs[i], out_bytes[i], ins[j], in_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    }
    if (total == 0) return 0;
    IcpDev p;
    p.fx = q->fx; p.fy = q->fy; p.cx = q->cx; p.cy = q->cy;
    p.ratio = q->depth_unit_ratio;
    p.max_distance = q->max_distance;
    for (int i = 0; i < 6; ++i) p.twist_p[i] = q->twist_p[i];
    p.height = q->height;
    p.width = q->width;
    double* sc = reinterpret_cast<double*>(scratch);
    hipStream_t s = as_stream(stream);
    return dispatch_depth(q->depth_dtype, [&](auto dt) {
        return launch_run<decltype(dt)>(q, p, live_depth, pred_depth, pred_normals, twist_inout, records, sc,
                                        residuals_out, (int)total, s);
    });
}

namespace {

PyrLevel pyr_level_of(const lsf_icp_pyramid_params* q, int level) {
    PyrLevel lv;
    lv.fx = q->fx; lv.fy = q->fy; lv.cx = q->cx; lv.cy = q->cy;
    lv.offset = 0;
    for (int l = 0; l < level; ++l) {  // lsf_depth_pyramid's level intrinsics and layout
        lv.offset += (long long)(q->height >> l) * (q->width >> l);
        lv.fx = lv.fx / 2.0;
        lv.fy = lv.fy / 2.0;
        lv.cx = (lv.cx - 0.5) / 2.0;
        lv.cy = (lv.cy - 0.5) / 2.0;
    }
    lv.ni = q->width >> level;
    lv.nj = q->height >> level;
    lv.tiles_x = (lv.ni + kTile - 1) / kTile;
    lv.tiles = lv.tiles_x * ((lv.nj + kTile - 1) / kTile);
    return lv;
}

template <int MODE, bool GATE>
int launch_pyramid(unsigned blocks, const float* live, const float* live_normals, const float* pred_depth,
                   const float* pred_normals, double* twist, double* records, double* scratch, float* residuals,
                   const IcpDev& p, const PyrLevel& lv, double cos_max, int k, int prev_blocks, int prev_level,
                   hipStream_t s) {
    hipLaunchKernelGGL((icp_pyramid_kernel<MODE, GATE>), dim3(blocks), dim3(kBlock), 0, s, live, live_normals,
                       pred_depth, pred_normals, twist, records, scratch, residuals, p, lv, cos_max, k, prev_blocks,
                       prev_level);
    return launch_status();
}

template <bool GATE>
int launch_run_pyramid(const lsf_icp_pyramid_params* q, const IcpDev& p, const float* live, const float* live_normals,
                       const float* pred_depth, const float* pred_normals, double* twist, double* records,
                       double* scratch, float* residuals, int total, hipStream_t s) {
    int k = 0, prev_blocks = 0, prev_level = 0;
    PyrLevel lv = pyr_level_of(q, 0);
    for (int l = 0; l < q->levels; ++l) {
        lv = pyr_level_of(q, q->levels - 1 - l);
        const int blocks = lv.tiles < kMaxBlocks ? lv.tiles : kMaxBlocks;
        for (int it = 0; it < q->iterations[l]; ++it, ++k) {
            if (int e = launch_pyramid<ITERATE, GATE>(blocks, live, live_normals, pred_depth, pred_normals, twist,
                                                      records, scratch, k == total - 1 ? residuals : nullptr, p, lv,
                                                      q->cos_max_angle, k, prev_blocks, prev_level, s))
                return e;
            prev_blocks = blocks;
            prev_level = l;
        }
    }
    return launch_pyramid<FINISH, GATE>(1, live, live_normals, pred_depth, pred_normals, twist, records, scratch,
                                        nullptr, p, lv, q->cos_max_angle, total, prev_blocks, prev_level, s);
}

}  // namespace

extern "C" int lsf_icp_run_pyramid(const float* live_depth, const float* live_normals, const float* pred_depth,
                                   const float* pred_normals, double* twist_inout, double* records, void* scratch,
                                   float* residuals_out, const lsf_icp_pyramid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !live_normals || !pred_depth || !pred_normals || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_icp_pyramid_params* q = params;
    if (q->height < 1 || q->width < 1 || (long long)q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    const double all[] = {q->fx, q->fy, q->cx, q->cy, q->twist_p[0], q->twist_p[1], q->twist_p[2], q->twist_p[3],
                          q->twist_p[4], q->twist_p[5]};
    for (double x : all)
        if (!std::isfinite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->max_distance > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (!(q->cos_max_angle >= -1.0 && q->cos_max_angle <= 1.0)) return LSF_ERR_BAD_ARGUMENT;
    if (q->pyramid_levels < 1 || q->pyramid_levels > LSF_ICP_MAX_LEVELS || q->levels < 1 ||
        q->levels > q->pyramid_levels || (q->height >> (q->pyramid_levels - 1)) < 1 ||
        (q->width >> (q->pyramid_levels - 1)) < 1)
        return LSF_ERR_BAD_ARGUMENT;
    long long total = 0;
    int last = 0;  // the pyramid level of the last iteration
    for (int l = 0; l < q->levels; ++l) {
        if (q->iterations[l] < 0) return LSF_ERR_BAD_ARGUMENT;
        total += q->iterations[l];
        if (q->iterations[l] > 0) last = q->levels - 1 - l;
    }
    if (total > 0x7fffffffll / kRecord || (total > 0 && !records)) return LSF_ERR_BAD_ARGUMENT;
    // no output may alias an input or another output
    size_t pyramid_pixels = 0;
    for (int l = 0; l < q->pyramid_levels; ++l) pyramid_pixels += (size_t)(q->height >> l) * (q->width >> l);
    const size_t pixels = (size_t)q->height * q->width;
    const void* outs[4] = {twist_inout, records, scratch, residuals_out};
    const size_t out_bytes[4] = {6 * 8, (size_t)total * kRecord * 8, LSF_ICP_PYRAMID_SCRATCH_BYTES,
                                 (size_t)(q->height >> last) * (q->width >> last) * 4};
    const void* ins[4] = {live_depth, live_normals, pred_depth, pred_normals};
    const size_t in_bytes[4] = {pyramid_pixels * 4, pyramid_pixels * 12, pixels * 4, pixels * 12};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j)
            if (overlaps(outs[i], out_bytes[i], ins[j], in_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    }
    if (total == 0) return 0;
    IcpDev p;
    p.fx = q->fx; p.fy = q->fy; p.cx = q->cx; p.cy = q->cy;
    p.ratio = 1.0;
    p.max_distance = q->max_distance;
    for (int i = 0; i < 6; ++i) p.twist_p[i] = q->twist_p[i];
    p.height = q->height;
    p.width = q->width;
    double* sc = reinterpret_cast<double*>(scratch);
    hipStream_t s = as_stream(stream);
    return q->angle_gate
               ? launch_run_pyramid<true>(q, p, live_depth, live_normals, pred_depth, pred_normals, twist_inout,
                                          records, sc, residuals_out, (int)total, s)
               : launch_run_pyramid<false>(q, p, live_depth, live_normals, pred_depth, pred_normals, twist_inout,
                                           records, sc, residuals_out, (int)total, s);
}
