// Point-to-SDF tracking of a live depth frame against the canonical TSDF itself (include/lsf_hip.h,
// lsf_point_sdf_run, lsf_point_sdf_run_photometric, lsf_point_sdf_run_pyramid): the tracker of Bylow et al. (RSS 2013),
// which the reference does not have.  The arithmetic is INTEGRATION.md section 3 ("Point-to-SDF tracking");
// tests/point_sdf_restatement.py and tests/point_sdf_colour_restatement.py restate it.  Every per-pixel step
// is one float64 operation in the order written there; -ffp-contract=off keeps products and sums separately rounded, so
// the residual images, the weight image and the counts equal the restatement bit for bit.
// The schedule is projective ICP's (lsf_icp_shared.h): iteration k's launch first combines iteration k-1's per-block
// partial sums, solves and composes the twist (the prologue), then one lane per pixel of the source's level, a wave
// per 8 x 8 block of them -- the 64 points of a wave land within a few voxels of each other, so their 16 gathers (8
// weights, 8 values; lsf_tsdf_sample.h) share cache lines --, a grid-stride loop over 16 x 16 tiles, the float64 sums
// in registers, one block reduction into this block's partial.  No float atomics, no in-launch hand-off: a rerun is
// bit-identical.
// There is no prediction image, no normal and no association: the pixel's world point is sampled in the model.
//   SdfSource<DT>               the strided pixels, 30 sums: ICP's 29 and the pixels with a depth and no valid sample
//   PyramidSource<false>        lsf_point_sdf_run_pyramid: every pixel of one level of lsf_depth_pyramid's output,
//                               back-projected with the level's intrinsics (lsf_icp_shared.h); the same 30 sums, no
//                               gate
//   SdfColourSource<S>          either of the two with the colour term: a pixel with a geometric pair samples the
//                               luminance of the colour volume at the same 8 corners and compares it with its own
//                               intensity (the live colour image's, or the level of lsf_intensity_pyramid's output),
//                               scaled by lambda into the same 27 sums, and two more: the photometric pairs and
//                               sum r_I^2 (record slots 59 and 60); 32 sums
//   RobustSource<S>             any of the four with every pair's rows scaled by the Huber or Tukey weight of its own
//                               residual; three more sums (sum w, sum w_I, the outliers), at most 35, and the weight
//                               image of the last iteration
// On the host lsf_point_sdf_run and lsf_point_sdf_run_photometric share run_strided; the levels, the rows of a term
// (add_rows) and the select over (colour term, loss) are lsf_icp_shared.h's.
#include "lsf_icp_shared.h"
#include "lsf_tsdf_sample.h"

namespace {

static_assert(LSF_POINT_SDF_SCRATCH_BYTES == 2 * kMaxBlocks * (kSums + 1 + kRobustSums) * 8,
              "two ping-pong buffers of kMaxBlocks partials of 33 sums");
static_assert(LSF_POINT_SDF_COLOUR_SCRATCH_BYTES == 2 * kMaxBlocks * (kSums + 1 + 2 + kRobustSums) * 8,
              "the same with the two photometric sums: 35");
// tests/test_point_sdf_host.py holds the ctypes mirror to the same numbers
static_assert(offsetof(lsf_point_sdf_params, depth) == 96 && offsetof(lsf_point_sdf_params, image_height) == 108 &&
              offsetof(lsf_point_sdf_params, depth_dtype) == 116 && offsetof(lsf_point_sdf_params, iterations) == 124 &&
              offsetof(lsf_point_sdf_params, strides) == 140 && offsetof(lsf_point_sdf_params, loss) == 156 &&
              sizeof(lsf_point_sdf_params) == 160, "lsf_point_sdf_params");
// the two new structs are lsf_point_sdf_params with the colour term's members behind it:
// tests/test_point_sdf_colour_host.py holds the ctypes mirrors to the same numbers
static_assert(offsetof(lsf_point_sdf_photometric_params, loss) == 156 &&
              offsetof(lsf_point_sdf_photometric_params, photometric_weight) == 160 &&
              offsetof(lsf_point_sdf_photometric_params, max_intensity_difference) == 168 &&
              offsetof(lsf_point_sdf_photometric_params, intensity_scale) == 176 &&
              sizeof(lsf_point_sdf_photometric_params) == 184, "lsf_point_sdf_photometric_params");
static_assert(offsetof(lsf_point_sdf_pyramid_params, loss) == 156 &&
              offsetof(lsf_point_sdf_pyramid_params, photometric_weight) == 160 &&
              offsetof(lsf_point_sdf_pyramid_params, max_intensity_difference) == 168 &&
              offsetof(lsf_point_sdf_pyramid_params, intensity_scale) == 176 &&
              offsetof(lsf_point_sdf_pyramid_params, pyramid_levels) == 184 &&
              sizeof(lsf_point_sdf_pyramid_params) == 192, "lsf_point_sdf_pyramid_params");

// the strided pixels of the live image; the sum behind ICP's 29 (a pyramid source's slot, record slot 58) counts the
// pixels that had a depth but no valid sample
template <typename DT>
struct SdfSource : StridedSource<DT> {
    using Layout = Sums<true, false, false>;
    static constexpr int K = Layout::K;
};

// what a colour source compares the model's luminance with: the pixel's own intensity
// the strided pixels: the live colour image's three bytes, unrounded
struct ColourImage {
    const uint8_t* live_colour;  // [height][width][3]
    template <typename Pixel>
    __device__ double observed(const IcpDev& p, Pixel px) const {
        const uint8_t* lc = live_colour + ((long long)px.v * p.width + px.u) * 3;
        return ((0.299 * (double)lc[0] + 0.587 * (double)lc[1]) + 0.114 * (double)lc[2]) / 255.0;
    }
};

// a pyramid level: the same level of the frame's lsf_intensity_pyramid output
struct IntensityLevel {
    const float* live_intensity;  // the level's [nj][ni]
    template <typename Pixel>
    __device__ double observed(const IcpDev&, Pixel px) const { return (double)live_intensity[px.at]; }
};

// BASE's pixels and pairs with the colour term; LIVE: ColourImage or IntensityLevel
template <typename BASE, typename LIVE>
struct SdfColourSource : BASE {
    using Layout = Sums<true, true, false>;
    static constexpr int K = Layout::K;
    static constexpr bool kPhoto = true;
    LIVE live;
    const float4* colour;  // the model's colour volume, one (R, G, B, W) record per voxel
    float* intensity;      // r_I of the launch, laid out like the residuals, or NULL: kept for the last iteration
    double lambda, max_difference;
};

struct SdfDev {
    double voxel, mu;  // metres: the voxel size and the truncation distance
    double off[3];     // array offset, voxels
};

// the colour term of a pixel that has a geometric pair (g: its world point, cell: where its SDF sample was taken): r_I,
// its scaled terms added to acc; NaN and nothing added when one of the 8 colour weights is not > 0 or |r_I| exceeds the
// gate.  The geometric rows are finished before this is called, so J_I takes J's registers
template <typename SRC>
__device__ __forceinline__ float colour_term(const SRC& src, typename SRC::Pixel px, const Volume& vol,
                                             const Cell& cell, const double (&g)[3], const IcpDev& p, const SdfDev& s,
                                             double (&acc)[SRC::K]) {
    long long c[8];
    cell_corners(vol, cell.at, c);
    float4 rec[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) rec[q] = src.colour[c[q]];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && rec[q].w > 0.0f;  // NaN is not > 0
    if (!ok) return NAN;
    double y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        y[q] = ((0.299 * (double)rec[q].x + 0.587 * (double)rec[q].y) + 0.114 * (double)rec[q].z) / 255.0;
    const double h[3] = {1.0 - cell.f[0], 1.0 - cell.f[1], 1.0 - cell.f[2]};  // the sample's own, bit for bit
    double Y = 0.0, dY[3];
    trilinear_gradient(y, cell.f, h, Y, dY);
    const double rI = Y - src.live.observed(p, px);
    if (!(fabs(rI) <= src.max_difference)) return NAN;  // NaN fails
    double gI[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) gI[a] = dY[a] / s.voxel;
    const double J[6] = {src.lambda * gI[0], src.lambda * gI[1], src.lambda * gI[2],
                         src.lambda * (g[1] * gI[2] - g[2] * gI[1]), src.lambda * (g[2] * gI[0] - g[0] * gI[2]),
                         src.lambda * (g[0] * gI[1] - g[1] * gI[0])};
    const double r = src.lambda * rI;
    if constexpr (SRC::kRobust) {  // w_I of the unscaled r_I on the lambda-scaled row and residual
        bool outlier;
        const double w = src.weight(rI, src.intensity_scale, outlier);
        add_rows<true>(J, r, w, acc);
        acc[SRC::Layout::kPhotoAt + 1] += (w * rI) * rI;
        acc[SRC::Layout::kRobustAt + 1] += w;
    } else {
        add_rows<false>(J, r, 1.0, acc);
        acc[SRC::Layout::kPhotoAt + 1] += rI * rI;
    }
    acc[SRC::Layout::kPhotoAt] += 1.0;
    return (float)rI;
}

// the live vertex vx (camera coordinates) against the model at the estimate e: its residual r, the pair's terms added
// to acc, when the pixel is a pair; NaN otherwise.  A pixel without a valid sample counts in acc[kSums].
// SRC::kRobust: the pair's terms are scaled by its weight w, which goes into weight; a pair with w = 0 still counts.
// SRC::kPhoto: a pixel with a pair also gets colour_term, its r_I into photo.
template <typename SRC>
__device__ __forceinline__ float accumulate_point(const SRC& src, typename SRC::Pixel px, const Volume& vol,
                                                  const double (&vx)[3], const double (&e)[12], const IcpDev& p,
                                                  const SdfDev& s, double (&acc)[SRC::K], float& photo,
                                                  float& weight) {
    double dv[3], g[3], q[3], d[3], grad[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dv[c] = vx[c] - e[c * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (e[c] * dv[0] + e[4 + c] * dv[1]) + e[8 + c] * dv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = g[c] / s.voxel - s.off[c];
    double phi = 0.0;
    Cell cell;
    if (!sample_gradient(vol, q[0], q[1], q[2], phi, d, cell)) {
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
    if constexpr (SRC::kRobust) {
        bool outlier;
        const double w = src.weight(r, src.scale, outlier);
        add_rows<true>(J, r, w, acc);
        acc[27] += (w * r) * r;
        acc[SRC::Layout::kRobustAt] += w;
        acc[SRC::Layout::kRobustAt + 2] += outlier ? 1.0 : 0.0;
        weight = (float)w;
    } else {
        add_rows<false>(J, r, 1.0, acc);
        acc[27] += r * r;
    }
    acc[28] += 1.0;
    if constexpr (SRC::kPhoto) photo = colour_term(src, px, vol, cell, g, p, s, acc);
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
        float res = NAN, photo = NAN, weight = NAN;
        if (d > 0.0) {  // NaN is not > 0
            double vx[3];
            src.vertex(p, px, d, vx);
            res = accumulate_point(src, px, vol, vx, e, p, s, acc, photo, weight);
        }
        if (residuals) src.store(residuals, p, px, res);  // the last iteration
        if constexpr (SRC::kPhoto)
            if (src.intensity) src.store(src.intensity, p, px, photo);
        if constexpr (SRC::kRobust)
            if (src.weights) src.store(src.weights, p, px, weight);
    }
    store_partial(acc, red, scratch + (size_t)(k & 1) * kMaxBlocks * K);
}

// the host checks the three parameter structs share: lsf_icp_run's of the camera, the image and the levels,
// lsf_raycast's of the volume, and the band.  STRIDED: the live image is a depth image read on strides
template <bool STRIDED, typename Q>
bool params_ok(const Q* q) {
    if (q->image_height < 1 || q->image_width < 1 || (long long)q->image_height * q->image_width > 0x7fffffffll)
        return false;
    if (q->depth < 2 || q->height < 2 || q->width < 2) return false;
    const double all[] = {q->fx, q->fy, q->cx, q->cy, STRIDED ? q->depth_unit_ratio : 1.0, q->voxel_size, q->offset_x,
                          q->offset_y, q->offset_z, q->narrow_band_width_voxels};
    for (double x : all)
        if (!std::isfinite(x)) return false;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->max_distance > 0.0) || !(q->voxel_size > 0.0) ||
        !(q->narrow_band_width_voxels > 0.0))
        return false;
    if (q->levels < 1 || q->levels > LSF_ICP_MAX_LEVELS) return false;
    if constexpr (STRIDED) {
        if (!depth_dtype_ok(q->depth_dtype)) return false;
        for (int l = 0; l < q->levels; ++l)
            if (q->strides[l] < 1) return false;
    }
    if (q->loss == LSF_POINT_SDF_LOSS_NONE) return true;
    return (q->loss == LSF_ICP_LOSS_HUBER || q->loss == LSF_ICP_LOSS_TUKEY) && q->scale > 0.0;  // NaN is not > 0
}

// the checks of the optional colour term (model: the colour volume, live: the frame's colour image or intensity
// pyramid, both or neither): 1 with the term, 0 without, -1 refused
template <typename Q>
int colour_term_of(const Q* q, const float* model, const void* live, const float* intensity_residuals_out) {
    if ((model == nullptr) != (live == nullptr)) return -1;
    if (!(std::isfinite(q->photometric_weight) && q->photometric_weight >= 0.0)) return -1;
    if (!(q->max_intensity_difference > 0.0)) return -1;  // NaN is not > 0
    if (q->loss != LSF_POINT_SDF_LOSS_NONE && !(q->intensity_scale > 0.0)) return -1;
    if (!model) return q->photometric_weight == 0.0 && !intensity_residuals_out ? 0 : -1;
    if ((uintptr_t)model % 16 != 0) return -1;  // a voxel's record is one 16-byte load
    return q->photometric_weight > 0.0 ? 1 : -1;
}

// what every launch of a run shares
struct SdfRun {
    Volume vol;
    const void* live;  // the source's Live type
    double* twist;
    double* records;
    double* scratch;
    float* residuals;
    IcpDev p;
    SdfDev s;
    int total;  // iterations, > 0
    hipStream_t stream;
};

template <typename Q>
SdfRun run_of(const Q* q, const float* tsdf, const float* weight, const void* live, double ratio, double* twist,
              double* records, void* scratch, float* residuals, long long total, void* stream) {
    SdfRun r = {{tsdf, weight, q->width, q->height, q->depth}, live, twist, records,
                reinterpret_cast<double*>(scratch), residuals, {}, {}, (int)total, as_stream(stream)};
    r.p.fx = q->fx; r.p.fy = q->fy; r.p.cx = q->cx; r.p.cy = q->cy;
    r.p.ratio = ratio;
    r.p.max_distance = q->max_distance;
    r.p.height = q->image_height;
    r.p.width = q->image_width;
    r.s = {q->voxel_size, q->narrow_band_width_voxels * q->voxel_size, {q->offset_x, q->offset_y, q->offset_z}};
    return r;
}

// the schedule (launch_schedule) over this file's iteration kernel: the residual images from launch total - 1
template <typename SourceOf>
int launch_run(const SdfRun& r, int levels, const int32_t* iterations, SourceOf source_of) {
    using SRC = decltype(source_of(0));
    return launch_schedule(levels, iterations, r.total, r.twist, r.records, r.scratch, r.stream, source_of,
                           [&](SRC src, int blocks, int k, int prev_blocks, int prev_level, bool last) {
        if constexpr (SRC::kPhoto)
            if (!last) src.intensity = nullptr;
        hipLaunchKernelGGL(point_sdf_iterate_kernel<SRC>, dim3(blocks), dim3(kBlock), 0, r.stream, src, r.vol,
                           reinterpret_cast<const typename SRC::Live*>(r.live) + src.offset, r.twist, r.records,
                           r.scratch, last ? r.residuals : nullptr, r.p, r.s, k, prev_blocks, prev_level);
    });
}

static_assert(LSF_POINT_SDF_LOSS_NONE == 0, "a Loss without a loss (lsf_icp_shared.h)");

// the optional colour term of a run: the model's colour volume, the frame's colour image or intensity pyramid, the
// image r_I goes to, and the term's three settings.  Without the term: colour NULL, lambda 0, both others inf
struct ColourTerm {
    const float* colour;
    const void* live;
    float* intensity_residuals_out;
    double photometric_weight, max_intensity_difference, intensity_scale;
};

// the launches of a checked run over level(l) with the optional colour term (live_of(level): its LIVE) and loss
template <typename Q, typename LevelOf, typename LiveOf>
int launch_configured(const SdfRun& r, const Q* q, const ColourTerm& c, float* weights_out, LevelOf level,
                      LiveOf live_of) {
    using BASE = decltype(level(0));
    using LIVE = decltype(live_of(level(0)));
    return launch_selected(
        c.colour != nullptr, {q->loss, q->scale, c.intensity_scale, weights_out},
        [&](auto source_of) { return launch_run(r, q->levels, q->iterations, source_of); }, level,
        [&](const BASE& base) {
            return SdfColourSource<BASE, LIVE>{base, live_of(base), reinterpret_cast<const float4*>(c.colour),
                                               c.intensity_residuals_out, c.photometric_weight,
                                               c.max_intensity_difference};
        });
}

// the strided run of lsf_point_sdf_run and lsf_point_sdf_run_photometric (scratch_bytes: the caller's
// LSF_*_SCRATCH_BYTES), after the caller's checks of the pointers and the colour term
template <typename Q>
int run_strided(const Q* q, const float* tsdf, const float* weight, const void* live_depth, double* twist_inout,
                double* records, void* scratch, size_t scratch_bytes, float* residuals_out, float* weights_out,
                const ColourTerm& c, void* stream) {
    if (!params_ok<true>(q) || (q->loss == LSF_POINT_SDF_LOSS_NONE && weights_out)) return LSF_ERR_BAD_ARGUMENT;
    const long long total = iteration_total(q->iterations, q->levels, records);
    if (total < 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t pixels = (size_t)q->image_height * q->image_width;
    const size_t voxels = (size_t)q->depth * q->height * q->width * 4;
    if (aliased({{twist_inout, 6 * 8}, {records, (size_t)total * kRecord * 8}, {scratch, scratch_bytes},
                 {residuals_out, pixels * 4}, {c.intensity_residuals_out, pixels * 4}, {weights_out, pixels * 4}},
                {{tsdf, voxels}, {weight, voxels}, {c.colour, voxels * 4},
                 {live_depth, pixels * kDepthBytes[q->depth_dtype]}, {c.live, pixels * 3}}))
        return LSF_ERR_BAD_ARGUMENT;
    if (total == 0) return 0;
    const SdfRun r = run_of(q, tsdf, weight, live_depth, q->depth_unit_ratio, twist_inout, records, scratch,
                            residuals_out, total, stream);
    return dispatch_depth(q->depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        return launch_configured(
            r, q, c, weights_out,
            [&](int l) { return SdfSource<DT>{strided_level<DT>(q->image_height, q->image_width, q->strides[l])}; },
            [&](const SdfSource<DT>&) { return ColourImage{reinterpret_cast<const uint8_t*>(c.live)}; });
    });
}

}  // namespace

extern "C" int lsf_point_sdf_run(const float* tsdf, const float* weight, const void* live_depth, double* twist_inout,
                                 double* records, void* scratch, float* residuals_out, float* weights_out,
                                 const lsf_point_sdf_params* params, void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || tsdf == weight || !live_depth || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    // the struct has no colour members: no term, and the loss weighs the geometric residual alone
    return run_strided(params, tsdf, weight, live_depth, twist_inout, records, scratch, LSF_POINT_SDF_SCRATCH_BYTES,
                       residuals_out, weights_out, {nullptr, nullptr, nullptr, 0.0, INFINITY, INFINITY}, stream);
}

extern "C" int lsf_point_sdf_run_photometric(const float* tsdf, const float* weight, const float* colour,
                                             const void* live_depth, const uint8_t* live_colour, double* twist_inout,
                                             double* records, void* scratch, float* residuals_out,
                                             float* intensity_residuals_out, float* weights_out,
                                             const lsf_point_sdf_photometric_params* params, void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || tsdf == weight || !live_depth || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_point_sdf_photometric_params* q = params;
    if (colour_term_of(q, colour, live_colour, intensity_residuals_out) < 0) return LSF_ERR_BAD_ARGUMENT;
    return run_strided(q, tsdf, weight, live_depth, twist_inout, records, scratch, LSF_POINT_SDF_COLOUR_SCRATCH_BYTES,
                       residuals_out, weights_out,
                       {colour, live_colour, intensity_residuals_out, q->photometric_weight,
                        q->max_intensity_difference, q->intensity_scale},
                       stream);
}

extern "C" int lsf_point_sdf_run_pyramid(const float* tsdf, const float* weight, const float* colour,
                                         const float* pyramid_depth, const float* pyramid_intensity,
                                         double* twist_inout, double* records, void* scratch, float* residuals_out,
                                         float* intensity_residuals_out, float* weights_out,
                                         const lsf_point_sdf_pyramid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || tsdf == weight || !pyramid_depth || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_point_sdf_pyramid_params* q = params;
    if (!params_ok<false>(q) || (q->loss == LSF_POINT_SDF_LOSS_NONE && weights_out)) return LSF_ERR_BAD_ARGUMENT;
    if (q->pyramid_levels < 1 || q->pyramid_levels > LSF_ICP_MAX_LEVELS || q->levels > q->pyramid_levels ||
        (q->image_height >> (q->pyramid_levels - 1)) < 1 || (q->image_width >> (q->pyramid_levels - 1)) < 1)
        return LSF_ERR_BAD_ARGUMENT;
    if (colour_term_of(q, colour, pyramid_intensity, intensity_residuals_out) < 0) return LSF_ERR_BAD_ARGUMENT;
    const long long total = iteration_total(q->iterations, q->levels, records);
    if (total < 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t levels_pixels = pyramid_pixels(q->image_height, q->image_width, q->pyramid_levels);
    const size_t last_bytes = last_level_pixels(q->image_height, q->image_width, q->levels, q->iterations) * 4;
    const size_t voxels = (size_t)q->depth * q->height * q->width * 4;
    if (aliased({{twist_inout, 6 * 8}, {records, (size_t)total * kRecord * 8},
                 {scratch, LSF_POINT_SDF_COLOUR_SCRATCH_BYTES}, {residuals_out, last_bytes},
                 {intensity_residuals_out, last_bytes}, {weights_out, last_bytes}},
                {{tsdf, voxels}, {weight, voxels}, {colour, voxels * 4}, {pyramid_depth, levels_pixels * 4},
                 {pyramid_intensity, levels_pixels * 4}}))
        return LSF_ERR_BAD_ARGUMENT;
    if (total == 0) return 0;
    const SdfRun r = run_of(q, tsdf, weight, pyramid_depth, 1.0, twist_inout, records, scratch, residuals_out, total,
                            stream);
    return launch_configured(
        r, q, {colour, pyramid_intensity, intensity_residuals_out, q->photometric_weight, q->max_intensity_difference,
               q->intensity_scale},
        weights_out,
        [&](int l) {
            return pyramid_level<false>(q->fx, q->fy, q->cx, q->cy, -1.0, q->image_height, q->image_width, q->levels, l);
        },
        [&](const PyramidSource<false>& level) { return IntensityLevel{pyramid_intensity + level.offset}; });
}
