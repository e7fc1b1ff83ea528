// Point-to-SDF tracking of a live depth frame against the canonical TSDF itself (include/lsf_hip.h,
// lsf_point_sdf_run): the tracker of Bylow et al. (RSS 2013), which the reference does not have.  The arithmetic is
// INTEGRATION.md section 3 ("Point-to-SDF tracking"); tests/point_sdf_restatement.py restates it.  Every per-pixel step
// is one float64 operation in the order written there; -ffp-contract=off keeps products and sums separately rounded, so
// the residual image, the weight image and the counts equal the restatement bit for bit.
// The schedule is projective ICP's (lsf_icp_shared.h): iteration k's launch first combines iteration k-1's per-block
// partial sums, solves and composes the twist (the prologue), then one lane per strided live pixel, a wave per 8 x 8
// block of them -- the 64 points of a wave land within a few voxels of each other, so their 16 gathers (8 weights, 8
// values; lsf_tsdf_sample.h) share cache lines --, a grid-stride loop over 16 x 16 tiles, the float64 sums in registers,
// one block reduction into this block's partial.  No float atomics, no in-launch hand-off: a rerun is bit-identical.
// There is no prediction image, no normal and no association: the pixel's world point is sampled in the model.
//   SdfSource<DT>               the strided pixels, 30 sums: ICP's 29 and the pixels with a depth and no valid sample
//   RobustSource<SdfSource<DT>> the same with every pair's rows scaled by the Huber or Tukey weight of its residual; 33
//                               sums (sum w, an unused sum w_I, the outliers) and the weight image of the last iteration
#include "lsf_icp_shared.h"
#include "lsf_tsdf_sample.h"

namespace {

static_assert(LSF_POINT_SDF_SCRATCH_BYTES == 2 * kMaxBlocks * (kSums + 1 + kRobustSums) * 8,
              "two ping-pong buffers of kMaxBlocks partials of 33 sums");
// tests/test_point_sdf_host.py holds the ctypes mirror to the same numbers
static_assert(offsetof(lsf_point_sdf_params, depth) == 96 && offsetof(lsf_point_sdf_params, image_height) == 108 &&
              offsetof(lsf_point_sdf_params, depth_dtype) == 116 && offsetof(lsf_point_sdf_params, iterations) == 124 &&
              offsetof(lsf_point_sdf_params, strides) == 140 && offsetof(lsf_point_sdf_params, loss) == 156 &&
              sizeof(lsf_point_sdf_params) == 160, "lsf_point_sdf_params");

// the strided pixels of the live image; the sum behind ICP's 29 (a pyramid source's slot, record slot 58) counts the
// pixels that had a depth but no valid sample
template <typename DT>
struct SdfSource : StridedSource<DT> {
    using Layout = Sums<true, false, false>;
    static constexpr int K = Layout::K;
};

struct SdfDev {
    double voxel, mu;  // metres: the voxel size and the truncation distance
    double off[3];     // array offset, voxels
};

// the live vertex vx (camera coordinates) against the model at the estimate e: its residual r, the pair's terms added
// to acc, when the pixel is a pair; NaN otherwise.  A pixel without a valid sample counts in acc[kSums].
// SRC::kRobust: the pair's terms are scaled by its weight w, which goes into weight; a pair with w = 0 still counts.
template <typename SRC>
__device__ __forceinline__ float accumulate_point(const SRC& src, const Volume& vol, const double (&vx)[3],
                                                  const double (&e)[12], const IcpDev& p, const SdfDev& s,
                                                  double (&acc)[SRC::K], float& weight) {
    double dv[3], g[3], q[3], d[3], grad[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dv[c] = vx[c] - e[c * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (e[c] * dv[0] + e[4 + c] * dv[1]) + e[8 + c] * dv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = g[c] / s.voxel - s.off[c];
    double phi = 0.0;
    if (!sample_gradient(vol, q[0], q[1], q[2], phi, d)) {
        acc[kSums] += 1.0;
        return NAN;
    }
    const double r = s.mu * phi;
    if (!(fabs(r) <= p.max_distance)) return NAN;  // NaN fails
#pragma unroll
    for (int c = 0; c < 3; ++c) grad[c] = (s.mu * d[c]) / s.voxel;
    if (!(grad[0] != 0.0 || grad[1] != 0.0 || grad[2] != 0.0)) return NAN;
    const double J[6] = {grad[0], grad[1], grad[2], g[1] * grad[2] - g[2] * grad[1], g[2] * grad[0] - g[0] * grad[2],
                         g[0] * grad[1] - g[1] * grad[0]};
    int n = 0;
    if constexpr (SRC::kRobust) {
        bool outlier;
        const double w = src.weight(r, src.scale, outlier);
        double wJ[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) wJ[a] = w * J[a];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[n++] += wJ[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] -= wJ[a] * r;
        acc[27] += (w * r) * r;
        acc[SRC::Layout::kRobustAt] += w;
        acc[SRC::Layout::kRobustAt + 2] += outlier ? 1.0 : 0.0;
        weight = (float)w;
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[n++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] -= J[a] * r;
        acc[27] += r * r;
    }
    acc[28] += 1.0;
    return (float)r;
}

template <typename SRC>
__global__ __launch_bounds__(kBlock) void point_sdf_iterate_kernel(SRC src, Volume vol,
                                                                   const typename SRC::Live* __restrict__ live,
                                                                   double* __restrict__ twist_io,
                                                                   double* __restrict__ records,
                                                                   double* __restrict__ scratch,
                                                                   float* __restrict__ residuals, IcpDev p, SdfDev s,
                                                                   int k, int prev_blocks, int prev_level) {
    constexpr int K = SRC::K;
    __shared__ double red[kBlock / kWave][K];
    __shared__ double tw[6], pose[12], pose_p[12];

    icp_prologue<typename SRC::Layout>(k, prev_blocks, prev_level, twist_io, records, scratch, red, tw, nullptr);
    double e[12], ep[12];  // ep: the camera of p.twist_p = 0, not read
    load_poses(tw, p, pose, pose_p, e, ep);

    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ox = (wave % (kTile / kSub)) * kSub + lane % kSub, oy = (wave / (kTile / kSub)) * kSub + lane / kSub;
    for (int tile = blockIdx.x; tile < src.grid.tiles; tile += gridDim.x) {
        const int i = (tile % src.grid.tiles_x) * kTile + ox, j = (tile / src.grid.tiles_x) * kTile + oy;
        if (i >= src.grid.ni || j >= src.grid.nj) continue;
        const auto px = src.pixel(i, j);
        const double d = src.depth(live, p, px);
        float res = NAN, weight = NAN;
        if (d > 0.0) {  // NaN is not > 0
            double vx[3];
            src.vertex(p, px, d, vx);
            res = accumulate_point(src, vol, vx, e, p, s, acc, weight);
        }
        if (residuals) src.store(residuals, p, px, res);  // the last iteration
        if constexpr (SRC::kRobust)
            if (src.weights) src.store(src.weights, p, px, weight);
    }
    store_partial(acc, red, scratch + (size_t)(k & 1) * kMaxBlocks * K);
}

// the host checks: lsf_icp_run's of the camera, the image and the levels, lsf_raycast's of the volume, and the band
bool params_ok(const lsf_point_sdf_params* q) {
    if (q->image_height < 1 || q->image_width < 1 || (long long)q->image_height * q->image_width > 0x7fffffffll)
        return false;
    if (q->depth < 2 || q->height < 2 || q->width < 2) return false;
    const double all[] = {q->fx, q->fy, q->cx, q->cy, q->depth_unit_ratio, q->voxel_size, q->offset_x, q->offset_y,
                          q->offset_z, q->narrow_band_width_voxels};
    for (double x : all)
        if (!std::isfinite(x)) return false;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->max_distance > 0.0) || !(q->voxel_size > 0.0) ||
        !(q->narrow_band_width_voxels > 0.0))
        return false;
    if (!depth_dtype_ok(q->depth_dtype) || q->levels < 1 || q->levels > LSF_ICP_MAX_LEVELS) return false;
    for (int l = 0; l < q->levels; ++l)
        if (q->strides[l] < 1) return false;
    if (q->loss == LSF_POINT_SDF_LOSS_NONE) return true;
    return (q->loss == LSF_ICP_LOSS_HUBER || q->loss == LSF_ICP_LOSS_TUKEY) && q->scale > 0.0;  // NaN is not > 0
}

}  // namespace

extern "C" int lsf_point_sdf_run(const float* tsdf, const float* weight, const void* live_depth, double* twist_inout,
                                 double* records, void* scratch, float* residuals_out, float* weights_out,
                                 const lsf_point_sdf_params* params, void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || tsdf == weight || !live_depth || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_point_sdf_params* q = params;
    if (!params_ok(q) || (q->loss == LSF_POINT_SDF_LOSS_NONE && weights_out)) return LSF_ERR_BAD_ARGUMENT;
    const long long total = iteration_total(q->iterations, q->levels, records);
    if (total < 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t pixels = (size_t)q->image_height * q->image_width;
    const size_t voxels = (size_t)q->depth * q->height * q->width * 4;
    if (aliased({{twist_inout, 6 * 8}, {records, (size_t)total * kRecord * 8}, {scratch, LSF_POINT_SDF_SCRATCH_BYTES},
                 {residuals_out, pixels * 4}, {weights_out, pixels * 4}},
                {{tsdf, voxels}, {weight, voxels}, {live_depth, pixels * kDepthBytes[q->depth_dtype]}}))
        return LSF_ERR_BAD_ARGUMENT;
    if (total == 0) return 0;
    IcpDev p = {};
    p.fx = q->fx; p.fy = q->fy; p.cx = q->cx; p.cy = q->cy;
    p.ratio = q->depth_unit_ratio;
    p.max_distance = q->max_distance;
    p.height = q->image_height;
    p.width = q->image_width;
    const SdfDev s = {q->voxel_size, q->narrow_band_width_voxels * q->voxel_size,
                      {q->offset_x, q->offset_y, q->offset_z}};
    const Volume vol{tsdf, weight, q->width, q->height, q->depth};
    double* const part = reinterpret_cast<double*>(scratch);
    hipStream_t st = as_stream(stream);
    return dispatch_depth(q->depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        auto level = [&](int l) {
            const int stride = q->strides[l];
            return SdfSource<DT>{{grid_of((q->image_width + stride - 1) / stride,
                                          (q->image_height + stride - 1) / stride), stride}};
        };
        auto run = [&](auto source_of) {
            using SRC = decltype(source_of(0));
            return launch_schedule(q->levels, q->iterations, (int)total, twist_inout, records, part, st, source_of,
                                   [&](SRC src, int blocks, int k, int prev_blocks, int prev_level, bool last) {
                hipLaunchKernelGGL(point_sdf_iterate_kernel<SRC>, dim3(blocks), dim3(kBlock), 0, st, src, vol,
                                   reinterpret_cast<const DT*>(live_depth), twist_inout, records, part,
                                   last ? residuals_out : nullptr, p, s, k, prev_blocks, prev_level);
            });
        };
        if (q->loss == LSF_POINT_SDF_LOSS_NONE) return run(level);
        return run([&](int l) {
            return RobustSource<SdfSource<DT>>{level(l), q->loss, q->scale, INFINITY, weights_out};
        });
    });
}
