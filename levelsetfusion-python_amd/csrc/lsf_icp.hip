// Projective point-to-plane ICP against the ray-cast prediction (include/lsf_hip.h, lsf_icp_run, lsf_icp_run_pyramid,
// lsf_icp_run_photometric and lsf_icp_run_pyramid_photometric): the KinectFusion tracker, which the reference does not
// have.  The arithmetic is INTEGRATION.md section 3 ("Projective ICP"); tests/icp_restatement.py restates it.  Every
// per-pixel step is one float64 operation in the order written there; -ffp-contract=off keeps products and sums
// separately rounded, so the residual image and the correspondence count equal the restatement bit for bit.  One
// iteration kernel over a live source, and the 3-D rigid tracker's schedule (lsf_rigid_solve.h):
//   iterate  iteration k: prologue = combine iteration k-1's per-block partial sums in a fixed order, solve the 6 x 6
//            system, compose the step into the twist (every block computes the same twist bit for bit, block 0 writes
//            record k-1); body = one lane per pixel of the source's level, a wave per 8 x 8 block of them, a
//            grid-stride loop over 16 x 16 tiles, the float64 sums kept in registers; one block reduction at the end
//            into this block's partial (ping-pong buffer k & 1)
//   finish   the prologue alone for the last iteration, one block; writes the final twist
// The partials cross launch boundaries only: no float atomics, no in-launch hand-off, so a rerun is bit-identical.
// A source is the level of a launch: its pixel grid, a pixel's camera-space vertex, and how the residual is stored.
//   StridedSource  lsf_icp_run: the pixels (stride i, stride j) of the live depth image, 29 sums
//   PyramidSource  lsf_icp_run_pyramid: every pixel of one level of lsf_depth_pyramid's output, back-projected with
//                  the level's intrinsics; an optional normal-angle gate after the distance test, and a 30th sum, the
//                  pairs the gate rejected (record slot 58)
//   PhotometricSource  lsf_icp_run_photometric: StridedSource's pixels; a pixel with a geometric pair also gets the
//                  intensity term of INTEGRATION.md section 3 ("Photometric ICP") against the ray-cast colour image,
//                  scaled by lambda into the same 27 sums, and two more: the photometric pairs and sum r_I^2 (record
//                  slots 59 and 60)
//   PyramidPhotometricSource  lsf_icp_run_pyramid_photometric: PyramidSource's pixels and gate; the intensity term is
//                  taken at the pixel's own level, between that level of two lsf_intensity_pyramid outputs (the live
//                  frame's and the prediction's) with the level's intrinsics; 32 sums, slots 58, 59 and 60
//   RobustSource<S>  lsf_icp_run_robust and lsf_icp_run_pyramid_robust: any of the four with every pair's rows scaled
//                  by a Huber or Tukey weight of its own residual ("Robust ICP";
//                  tests/robust_icp_restatement.py); the loss is a wave-uniform run-time select; three more sums: sum w,
//                  sum w_I and the geometric outliers (record slots 61, 62 and 63), and the weight image of the last
//                  iteration beside the residuals
// What this file shares with the point-to-SDF tracker (lsf_point_sdf.hip) -- the sums' layout, StridedSource,
// PyramidSource and their levels, RobustSource, add_rows, compose, the prologue, load_poses, the finishing kernel, the
// schedule, launch_selected, the host checks -- is in lsf_icp_shared.h.
// On the host the six entry points are two runs, run_strided and run_pyramid, over one Settings filled from any of the
// six parameter structs (settings_of) and one Images of pointers; an entry point keeps its required pointers and its
// rule for the intensity term.
#include <type_traits>

#include "lsf_icp_shared.h"

namespace {

constexpr int kPyrSums = 30;  // lsf_icp_run_pyramid: and the pairs the angle gate rejected
constexpr int kPhotoSums = 31;  // lsf_icp_run_photometric: kSums, then the photometric pairs and sum r_I^2
constexpr int kPyrPhotoSums = 32;  // lsf_icp_run_pyramid_photometric: kPyrSums, then the same two
static_assert(LSF_ICP_SCRATCH_BYTES == 2 * kMaxBlocks * kSums * 8, "two ping-pong buffers of kMaxBlocks partials");
static_assert(LSF_ICP_PYRAMID_SCRATCH_BYTES == 2 * kMaxBlocks * kPyrSums * 8, "the same with the 30th sum");
static_assert(LSF_ICP_PHOTOMETRIC_SCRATCH_BYTES == 2 * kMaxBlocks * kPhotoSums * 8, "the same with 31 sums");
static_assert(LSF_ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES == 2 * kMaxBlocks * kPyrPhotoSums * 8, "the same with 32 sums");
static_assert(LSF_ICP_ROBUST_SCRATCH_BYTES == 2 * kMaxBlocks * (kPhotoSums + kRobustSums) * 8, "the same with 34 sums");
static_assert(LSF_ICP_PYRAMID_ROBUST_SCRATCH_BYTES == 2 * kMaxBlocks * (kPyrPhotoSums + kRobustSums) * 8, "the same with 35 sums");
// the robust structs are the photometric ones with the loss behind them: tests/test_robust_icp_host.py holds the
// ctypes mirrors to the same numbers
static_assert(sizeof(lsf_icp_photometric_params) == 160 && offsetof(lsf_icp_robust_params, loss) == 160 &&
              offsetof(lsf_icp_robust_params, scale) == 168 && offsetof(lsf_icp_robust_params, intensity_scale) == 176 &&
              sizeof(lsf_icp_robust_params) == 184, "lsf_icp_robust_params");
static_assert(sizeof(lsf_icp_pyramid_photometric_params) == 152 && offsetof(lsf_icp_pyramid_robust_params, loss) == 152 &&
              offsetof(lsf_icp_pyramid_robust_params, scale) == 160 &&
              offsetof(lsf_icp_pyramid_robust_params, intensity_scale) == 168 &&
              sizeof(lsf_icp_pyramid_robust_params) == 176, "lsf_icp_pyramid_robust_params");

static_assert(Sums<false, false, false>::K == kSums && Sums<true, false, false>::K == kPyrSums &&
              Sums<false, true, false>::K == kPhotoSums && Sums<true, true, false>::K == kPyrPhotoSums,
              "the four plain sources keep their sums");

// What photometric_term asks of a source with kPhoto: the image the term is taken in -- its intrinsics and extents,
// the pixel's unrounded projection into it, the prediction's intensity at one of its pixels -- and the live pixel's own
// intensity; the last two sums of its K are the photometric pairs and sum r_I^2.

// lsf_icp_run_photometric: the strided pixels; the term is taken in the full-resolution prediction
template <typename DT>
struct PhotometricSource : StridedSource<DT> {
    using Pixel = typename StridedSource<DT>::Pixel;
    using Layout = Sums<false, true, false>;
    static constexpr int K = Layout::K;
    static constexpr bool kPhoto = true;
    const uint8_t* live_colour;  // [height][width][3]
    const float* pred_colour;    // [height][width][4], Y last
    float* intensity;            // r_I of the launch, or NULL: launch_run keeps it for the last iteration
    double lambda, max_difference;

    __device__ double photo_fx(const IcpDev& p) const { return p.fx; }
    __device__ double photo_fy(const IcpDev& p) const { return p.fy; }
    __device__ int photo_width(const IcpDev& p) const { return p.width; }
    __device__ int photo_height(const IcpDev& p) const { return p.height; }
    // the geometric pair's own projection, before rint
    __device__ void project(const IcpDev&, const double (&)[3], double pu, double pv, double& iu, double& iv) const {
        iu = pu;
        iv = pv;
    }
    __device__ double predicted(long long at) const { return (double)pred_colour[at * 4 + 3]; }
    __device__ double observed(const IcpDev& p, Pixel px) const {
        const uint8_t* lc = live_colour + ((long long)px.v * p.width + px.u) * 3;
        return ((0.299 * (double)lc[0] + 0.587 * (double)lc[1]) + 0.114 * (double)lc[2]) / 255.0;
    }
};

// lsf_icp_run_pyramid_photometric: the pixels of one pyramid level; the term is taken in that level of the
// prediction's intensity pyramid, against the same level of the live one
template <bool GATE>
struct PyramidPhotometricSource : PyramidSource<GATE> {
    using Pixel = typename PyramidSource<GATE>::Pixel;
    using Layout = Sums<true, true, false>;
    static constexpr int K = Layout::K;
    static constexpr bool kPhoto = true;
    const float* live_intensity;  // the level's [nj][ni] of the live frame's lsf_intensity_pyramid output
    const float* pred_intensity;  // the same level of the prediction's
    float* intensity;             // r_I of the launch at the level's extents, or NULL
    double lambda, max_difference;

    __device__ double photo_fx(const IcpDev&) const { return this->fx; }
    __device__ double photo_fy(const IcpDev&) const { return this->fy; }
    __device__ int photo_width(const IcpDev&) const { return this->grid.ni; }
    __device__ int photo_height(const IcpDev&) const { return this->grid.nj; }
    __device__ void project(const IcpDev&, const double (&q)[3], double, double, double& iu, double& iv) const {
        iu = (this->fx * q[0]) / q[2] + this->cx;
        iv = (this->fy * q[1]) / q[2] + this->cy;
    }
    __device__ double predicted(long long at) const { return (double)pred_intensity[at]; }
    __device__ double observed(const IcpDev&, Pixel px) const { return (double)live_intensity[px.at]; }
};

// the intensity term of a pixel that has a geometric pair (q: its point in the prediction's camera, before the
// projection is rounded, (gu, gv) that projection; g: its world point): r_I, its scaled terms added to acc; NaN and
// nothing added when the 2 x 2 neighbourhood leaves the source's intensity image, one of its four Y is not finite, or
// |r_I| exceeds the gate
template <typename SRC>
__device__ __forceinline__ float photometric_term(const SRC& src, typename SRC::Pixel px, double gu, double gv,
                                                  const double (&q)[3], const double (&g)[3], const double (&ep)[12],
                                                  const IcpDev& p, double (&acc)[SRC::K]) {
    double pu, pv;
    src.project(p, q, gu, gv, pu, pv);
    const int width = src.photo_width(p), height = src.photo_height(p);
    const double x0 = floor(pu), y0 = floor(pv);
    // compared as doubles first: NaN and far-off values never reach the integer conversion
    if (!(0.0 <= x0 && x0 + 1.0 <= (double)(width - 1) && 0.0 <= y0 && y0 + 1.0 <= (double)(height - 1)))
        return NAN;
    const long long at = (long long)(int)y0 * width + (int)x0;
    const double I00 = src.predicted(at), I10 = src.predicted(at + 1);
    const double I01 = src.predicted(at + width);
    const double I11 = src.predicted(at + width + 1);
    if (!(isfinite(I00) && isfinite(I10) && isfinite(I01) && isfinite(I11))) return NAN;
    const double al = pu - x0, be = pv - y0;
    const double ha = 1.0 - al, hb = 1.0 - be;
    const double Ip = hb * (ha * I00 + al * I10) + be * (ha * I01 + al * I11);
    const double Iu = hb * (I10 - I00) + be * (I11 - I01);
    const double Iv = ha * (I01 - I00) + al * (I11 - I10);
    const double Il = src.observed(p, px);
    const double rI = Ip - Il;
    if (!(fabs(rI) <= src.max_difference)) return NAN;
    const double su = Iu * src.photo_fx(p), sv = Iv * src.photo_fy(p);
    const double c[3] = {su / q[2], sv / q[2], -((su * q[0] + sv * q[1]) / (q[2] * q[2]))};
    double a[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = (ep[j] * c[0] + ep[4 + j] * c[1]) + ep[8 + j] * c[2];
    const double J[6] = {src.lambda * a[0], src.lambda * a[1], src.lambda * a[2],
                         src.lambda * (g[1] * a[2] - g[2] * a[1]), src.lambda * (g[2] * a[0] - g[0] * a[2]),
                         src.lambda * (g[0] * a[1] - g[1] * a[0])};
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

// the live vertex vx (camera coordinates) of the source's pixel px against the prediction at the estimate e: its
// residual r, the pair's terms added to acc, when the pair is valid and (SRC::kGate) the live normal passes the angle
// gate; NaN otherwise.  A pair that passes the distance test and fails the gate counts in acc[kSums].  SRC::kPhoto:
// a pixel with a pair also gets photometric_term, its r_I into photo.  SRC::kRobust: the pair's terms are scaled by
// its weight w, which goes into weight; a pair with w = 0 still counts.
template <typename SRC>
__device__ __forceinline__ float accumulate_pair(const SRC& src, const float* __restrict__ live_normals,
                                                 typename SRC::Pixel px, const double (&vx)[3],
                                                 const double (&e)[12], const double (&ep)[12], const IcpDev& p,
                                                 const float* __restrict__ pred_depth,
                                                 const float* __restrict__ pred_normals, double (&acc)[SRC::K],
                                                 float& photo, float& weight) {
    double dv[3], g[3], q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dv[c] = vx[c] - e[c * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (e[c] * dv[0] + e[4 + c] * dv[1]) + e[8 + c] * dv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((ep[c * 4] * g[0] + ep[c * 4 + 1] * g[1]) + ep[c * 4 + 2] * g[2]) + ep[c * 4 + 3];
    if (!(q[2] > 0.0)) return NAN;
    const double pu = (p.fx * q[0]) / q[2] + p.cx, pv = (p.fy * q[1]) / q[2] + p.cy;
    const double fu = rint(pu), fv = rint(pv);
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
    if constexpr (SRC::kGate) {  // the live normal in world directions, m = R^T n, against N_w
        const float* nl = src.normal(live_normals, px);
        const double ln[3] = {(double)nl[0], (double)nl[1], (double)nl[2]};
        bool keep = ln[0] != 0.0 || ln[1] != 0.0 || ln[2] != 0.0;
        if (keep) {
            double m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = (e[c] * ln[0] + e[4 + c] * ln[1]) + e[8 + c] * ln[2];
            keep = (m[0] * Nw[0] + m[1] * Nw[1]) + m[2] * Nw[2] >= src.cos_max;
        }
        if (!keep) {
            acc[kSums] += 1.0;
            return NAN;
        }
    }
    const double r = (Nw[0] * diff[0] + Nw[1] * diff[1]) + Nw[2] * diff[2];
    const double J[6] = {Nw[0], Nw[1], Nw[2], g[1] * Nw[2] - g[2] * Nw[1], g[2] * Nw[0] - g[0] * Nw[2],
                         g[0] * Nw[1] - g[1] * Nw[0]};
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
    if constexpr (SRC::kPhoto) photo = photometric_term(src, px, pu, pv, q, g, ep, p, acc);
    return (float)r;
}

template <typename SRC>
__global__ __launch_bounds__(kBlock) void icp_iterate_kernel(SRC src, const typename SRC::Live* __restrict__ live,
                                                             const float* __restrict__ live_normals,
                                                             const float* __restrict__ pred_depth,
                                                             const float* __restrict__ pred_normals,
                                                             double* __restrict__ twist_io, double* __restrict__ records,
                                                             double* __restrict__ scratch, float* __restrict__ residuals,
                                                             IcpDev p, int k, int prev_blocks, int prev_level) {
    constexpr int K = SRC::K;
    __shared__ double red[kBlock / kWave][K];
    __shared__ double tw[6], pose[12], pose_p[12];

    icp_prologue<typename SRC::Layout>(k, prev_blocks, prev_level, twist_io, records, scratch, red, tw, nullptr);
    double e[12], ep[12];
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
            res = accumulate_pair(src, live_normals, px, vx, e, ep, p, pred_depth, pred_normals, acc, photo,
                                  weight);
        }
        if (residuals) src.store(residuals, p, px, res);  // the last iteration
        if constexpr (SRC::kPhoto)
            if (src.intensity) src.store(src.intensity, p, px, photo);
        if constexpr (SRC::kRobust)
            if (src.weights) src.store(src.weights, p, px, weight);
    }
    store_partial(acc, red, scratch + (size_t)(k & 1) * kMaxBlocks * K);
}

constexpr int kNoLoss = 0;  // a Settings without weights: no loss code an entry point accepts
static_assert(kNoLoss != LSF_ICP_LOSS_HUBER && kNoLoss != LSF_ICP_LOSS_TUKEY, "no loss is not a loss");

// what a run reads of its parameter struct: the union of the six public structs.  settings_of fills it from any of
// them, and the members a struct lacks get the neutral value: lambda 0, the gate inf, no loss, the scales inf.  The
// strided run reads depth_unit_ratio, depth_dtype and strides, the pyramid run cos_max_angle, pyramid_levels and
// angle_gate
struct Settings {
    double fx, fy, cx, cy, max_distance, twist_p[6];
    int height, width, levels;
    int32_t iterations[LSF_ICP_MAX_LEVELS];
    double depth_unit_ratio;
    int depth_dtype;
    int32_t strides[LSF_ICP_MAX_LEVELS];
    double cos_max_angle;
    int pyramid_levels, angle_gate;
    double photometric_weight, max_intensity_difference;
    Loss loss;  // weights_out: the run's
};

template <typename Q, typename = void> struct is_pyramid : std::false_type {};
template <typename Q> struct is_pyramid<Q, std::void_t<decltype(Q::pyramid_levels)>> : std::true_type {};
template <typename Q, typename = void> struct has_term : std::false_type {};
template <typename Q> struct has_term<Q, std::void_t<decltype(Q::photometric_weight)>> : std::true_type {};
template <typename Q, typename = void> struct has_loss : std::false_type {};
template <typename Q> struct has_loss<Q, std::void_t<decltype(Q::loss)>> : std::true_type {};

template <typename Q>
Settings settings_of(const Q* q, float* weights_out) {
    Settings s = {q->fx, q->fy, q->cx, q->cy, q->max_distance, {}, q->height, q->width, q->levels, {}, 1.0, 0, {},
                  -1.0, 0, 0, 0.0, INFINITY, {kNoLoss, INFINITY, INFINITY, weights_out}};
    for (int i = 0; i < 6; ++i) s.twist_p[i] = q->twist_p[i];
    for (int l = 0; l < LSF_ICP_MAX_LEVELS; ++l) s.iterations[l] = q->iterations[l];
    if constexpr (is_pyramid<Q>::value) {
        s.cos_max_angle = q->cos_max_angle;
        s.pyramid_levels = q->pyramid_levels;
        s.angle_gate = q->angle_gate;
    } else {
        s.depth_unit_ratio = q->depth_unit_ratio;
        s.depth_dtype = q->depth_dtype;
        for (int l = 0; l < LSF_ICP_MAX_LEVELS; ++l) s.strides[l] = q->strides[l];
    }
    if constexpr (has_term<Q>::value) {
        s.photometric_weight = q->photometric_weight;
        s.max_intensity_difference = q->max_intensity_difference;
    }
    if constexpr (has_loss<Q>::value) {
        s.loss.loss = q->loss;
        s.loss.scale = q->scale;
        s.loss.intensity_scale = q->intensity_scale;
    }
    return s;
}

// a run's pointers, the absent ones NULL.  live_term and pred_term: the two images of the intensity term, the strided
// run's uint8 colour image and float32 [h][w][4] prediction, the pyramid run's two float32 intensity pyramids
struct Images {
    const void* live_depth;
    const float* live_normals;
    const void* live_term;
    const float *pred_depth, *pred_normals, *pred_term;
    double *twist, *records;
    void* scratch;
    float *residuals_out, *intensity_residuals_out;
};

// what every launch of a run shares
struct Run {
    const void* live;           // the source's Live type
    const float* live_normals;  // NULL on the strided path
    const float* pred_depth;
    const float* pred_normals;
    double* twist;
    double* records;
    double* scratch;
    float* residuals;
    IcpDev p;
    int total;  // iterations, > 0
    hipStream_t stream;
};

// the schedule (launch_schedule) over this file's iteration kernel: the residuals from launch total - 1
template <typename SourceOf>
int launch_run(const Run& r, int levels, const int32_t* iterations, SourceOf source_of) {
    using SRC = decltype(source_of(0));
    return launch_schedule(levels, iterations, r.total, r.twist, r.records, r.scratch, r.stream, source_of,
                           [&](SRC src, int blocks, int k, int prev_blocks, int prev_level, bool last) {
        if constexpr (SRC::kPhoto)  // like the residuals: from the last iteration only
            if (!last) src.intensity = nullptr;
        hipLaunchKernelGGL(icp_iterate_kernel<SRC>, dim3(blocks), dim3(kBlock), 0, r.stream, src,
                           reinterpret_cast<const typename SRC::Live*>(r.live) + src.offset,
                           r.live_normals + src.offset * 3, r.pred_depth, r.pred_normals, r.twist, r.records,
                           r.scratch, last ? r.residuals : nullptr, r.p, k, prev_blocks, prev_level);
    });
}

// the checks every run shares: the extents, finite intrinsics and twist_p, max_distance
bool camera_ok(const Settings& q) {
    if (q.height < 1 || q.width < 1 || (long long)q.height * q.width > 0x7fffffffll) return false;
    const double all[] = {q.fx, q.fy, q.cx, q.cy, q.twist_p[0], q.twist_p[1], q.twist_p[2], q.twist_p[3],
                          q.twist_p[4], q.twist_p[5]};
    for (double x : all)
        if (!std::isfinite(x)) return false;
    return q.fx != 0.0 && q.fy != 0.0 && q.max_distance > 0.0;
}

Run run_of(const Settings& q, const Images& m, long long total, void* stream) {
    Run r = {m.live_depth, m.live_normals, m.pred_depth, m.pred_normals, m.twist, m.records,
             reinterpret_cast<double*>(m.scratch), m.residuals_out, {}, (int)total, as_stream(stream)};
    r.p.fx = q.fx; r.p.fy = q.fy; r.p.cx = q.cx; r.p.cy = q.cy;
    r.p.ratio = q.depth_unit_ratio;
    r.p.max_distance = q.max_distance;
    for (int i = 0; i < 6; ++i) r.p.twist_p[i] = q.twist_p[i];
    r.p.height = q.height;
    r.p.width = q.width;
    return r;
}

// the strided run of the three strided entry points (scratch_bytes: the caller's LSF_*_SCRATCH_BYTES): the checks of
// the settings, the alias check, and the launches over the source that the term (live_term) and the loss select
int run_strided(const Settings& q, const Images& m, size_t scratch_bytes, void* stream) {
    if (!camera_ok(q) || !std::isfinite(q.depth_unit_ratio) || !depth_dtype_ok(q.depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    if (q.levels < 1 || q.levels > LSF_ICP_MAX_LEVELS) return LSF_ERR_BAD_ARGUMENT;
    for (int l = 0; l < q.levels; ++l)
        if (q.strides[l] < 1) return LSF_ERR_BAD_ARGUMENT;
    const long long total = iteration_total(q.iterations, q.levels, m.records);
    if (total < 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t pixels = (size_t)q.height * q.width;
    if (aliased({{m.twist, 6 * 8}, {m.records, (size_t)total * kRecord * 8}, {m.scratch, scratch_bytes},
                 {m.residuals_out, pixels * 4}, {m.intensity_residuals_out, pixels * 4},
                 {q.loss.weights_out, pixels * 4}},
                {{m.live_depth, pixels * kDepthBytes[q.depth_dtype]}, {m.live_term, pixels * 3},
                 {m.pred_depth, pixels * 4}, {m.pred_normals, pixels * 12}, {m.pred_term, pixels * 16}}))
        return LSF_ERR_BAD_ARGUMENT;
    if (total == 0) return 0;
    const Run r = run_of(q, m, total, stream);
    return dispatch_depth(q.depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        return launch_selected(
            m.live_term != nullptr, q.loss,
            [&](auto source_of) { return launch_run(r, q.levels, q.iterations, source_of); },
            [&](int l) { return strided_level<DT>(q.height, q.width, q.strides[l]); },
            [&](const StridedSource<DT>& level) {
                return PhotometricSource<DT>{level, reinterpret_cast<const uint8_t*>(m.live_term), m.pred_term,
                                             m.intensity_residuals_out, q.photometric_weight,
                                             q.max_intensity_difference};
            });
    });
}

// the same for the three pyramid entry points
int run_pyramid(const Settings& q, const Images& m, size_t scratch_bytes, void* stream) {
    if (!camera_ok(q) || !(q.cos_max_angle >= -1.0 && q.cos_max_angle <= 1.0)) return LSF_ERR_BAD_ARGUMENT;
    if (q.pyramid_levels < 1 || q.pyramid_levels > LSF_ICP_MAX_LEVELS || q.levels < 1 ||
        q.levels > q.pyramid_levels || (q.height >> (q.pyramid_levels - 1)) < 1 ||
        (q.width >> (q.pyramid_levels - 1)) < 1)
        return LSF_ERR_BAD_ARGUMENT;
    const long long total = iteration_total(q.iterations, q.levels, m.records);
    if (total < 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t levels_pixels = pyramid_pixels(q.height, q.width, q.pyramid_levels);
    const size_t pixels = (size_t)q.height * q.width;
    const size_t last_bytes = last_level_pixels(q.height, q.width, q.levels, q.iterations) * 4;
    if (aliased({{m.twist, 6 * 8}, {m.records, (size_t)total * kRecord * 8}, {m.scratch, scratch_bytes},
                 {m.residuals_out, last_bytes}, {m.intensity_residuals_out, last_bytes},
                 {q.loss.weights_out, last_bytes}},
                {{m.live_depth, levels_pixels * 4}, {m.live_normals, levels_pixels * 12},
                 {m.live_term, levels_pixels * 4}, {m.pred_depth, pixels * 4}, {m.pred_normals, pixels * 12},
                 {m.pred_term, levels_pixels * 4}}))
        return LSF_ERR_BAD_ARGUMENT;
    if (total == 0) return 0;
    const Run r = run_of(q, m, total, stream);
    auto run = [&](auto gate) {
        constexpr bool GATE = decltype(gate)::value;
        return launch_selected(
            m.live_term != nullptr, q.loss,
            [&](auto source_of) { return launch_run(r, q.levels, q.iterations, source_of); },
            [&](int l) {
                return pyramid_level<GATE>(q.fx, q.fy, q.cx, q.cy, q.cos_max_angle, q.height, q.width, q.levels, l);
            },
            [&](const PyramidSource<GATE>& level) {
                return PyramidPhotometricSource<GATE>{level,
                                                      reinterpret_cast<const float*>(m.live_term) + level.offset,
                                                      m.pred_term + level.offset, m.intensity_residuals_out,
                                                      q.photometric_weight, q.max_intensity_difference};
            });
    };
    return q.angle_gate ? run(std::true_type()) : run(std::false_type());
}

// the photometric entry points' rule: lambda finite and > 0, the gate > 0 (NaN is not)
template <typename Q>
bool term_ok(const Q* q) {
    return std::isfinite(q->photometric_weight) && q->photometric_weight > 0.0 && q->max_intensity_difference > 0.0;
}

// the robust entry points' rule: the loss, both scales, and the optional intensity term (a, b: its two images, both or
// neither; without them lambda is 0 and there is no intensity residual image)
template <typename Q>
bool robust_term(const Q* q, const void* a, const void* b, const float* intensity_residuals_out) {
    if (q->loss != LSF_ICP_LOSS_HUBER && q->loss != LSF_ICP_LOSS_TUKEY) return false;
    if (!(q->scale > 0.0 && q->intensity_scale > 0.0)) return false;  // NaN is not > 0
    if ((a == nullptr) != (b == nullptr)) return false;
    if (!a) return q->photometric_weight == 0.0 && !intensity_residuals_out;
    return term_ok(q);
}

}  // namespace

// Each entry point keeps what is its own -- the pointers it requires and its rule for the intensity term -- and hands
// its settings, its pointers and its scratch size to the run of its source.

extern "C" int lsf_icp_run(const void* live_depth, const float* pred_depth, const float* pred_normals,
                           double* twist_inout, double* records, void* scratch, float* residuals_out,
                           const lsf_icp_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !pred_depth || !pred_normals || !twist_inout || !scratch || !params) return LSF_ERR_BAD_ARGUMENT;
    return run_strided(settings_of(params, nullptr),
                       {live_depth, nullptr, nullptr, pred_depth, pred_normals, nullptr, twist_inout, records, scratch,
                        residuals_out, nullptr},
                       LSF_ICP_SCRATCH_BYTES, stream);
}

extern "C" int lsf_icp_run_photometric(const void* live_depth, const uint8_t* live_colour, const float* pred_depth,
                                       const float* pred_normals, const float* pred_colour, double* twist_inout,
                                       double* records, void* scratch, float* residuals_out,
                                       float* intensity_residuals_out, const lsf_icp_photometric_params* params,
                                       void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !live_colour || !pred_depth || !pred_normals || !pred_colour || !twist_inout || !scratch ||
        !params || !term_ok(params))
        return LSF_ERR_BAD_ARGUMENT;
    return run_strided(settings_of(params, nullptr),
                       {live_depth, nullptr, live_colour, pred_depth, pred_normals, pred_colour, twist_inout, records,
                        scratch, residuals_out, intensity_residuals_out},
                       LSF_ICP_PHOTOMETRIC_SCRATCH_BYTES, stream);
}

extern "C" int lsf_icp_run_robust(const void* live_depth, const uint8_t* live_colour, const float* pred_depth,
                                  const float* pred_normals, const float* pred_colour, double* twist_inout,
                                  double* records, void* scratch, float* residuals_out,
                                  float* intensity_residuals_out, float* weights_out,
                                  const lsf_icp_robust_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !pred_depth || !pred_normals || !twist_inout || !scratch || !params ||
        !robust_term(params, live_colour, pred_colour, intensity_residuals_out))
        return LSF_ERR_BAD_ARGUMENT;
    return run_strided(settings_of(params, weights_out),
                       {live_depth, nullptr, live_colour, pred_depth, pred_normals, pred_colour, twist_inout, records,
                        scratch, residuals_out, intensity_residuals_out},
                       LSF_ICP_ROBUST_SCRATCH_BYTES, stream);
}

extern "C" int lsf_icp_run_pyramid(const float* live_depth, const float* live_normals, const float* pred_depth,
                                   const float* pred_normals, double* twist_inout, double* records, void* scratch,
                                   float* residuals_out, const lsf_icp_pyramid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !live_normals || !pred_depth || !pred_normals || !twist_inout || !scratch || !params)
        return LSF_ERR_BAD_ARGUMENT;
    return run_pyramid(settings_of(params, nullptr),
                       {live_depth, live_normals, nullptr, pred_depth, pred_normals, nullptr, twist_inout, records,
                        scratch, residuals_out, nullptr},
                       LSF_ICP_PYRAMID_SCRATCH_BYTES, stream);
}

extern "C" int lsf_icp_run_pyramid_photometric(const float* live_depth, const float* live_normals,
                                               const float* live_intensity, const float* pred_depth,
                                               const float* pred_normals, const float* pred_intensity,
                                               double* twist_inout, double* records, void* scratch,
                                               float* residuals_out, float* intensity_residuals_out,
                                               const lsf_icp_pyramid_photometric_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !live_normals || !live_intensity || !pred_depth || !pred_normals || !pred_intensity ||
        !twist_inout || !scratch || !params || !term_ok(params))
        return LSF_ERR_BAD_ARGUMENT;
    return run_pyramid(settings_of(params, nullptr),
                       {live_depth, live_normals, live_intensity, pred_depth, pred_normals, pred_intensity,
                        twist_inout, records, scratch, residuals_out, intensity_residuals_out},
                       LSF_ICP_PYRAMID_PHOTOMETRIC_SCRATCH_BYTES, stream);
}

extern "C" int lsf_icp_run_pyramid_robust(const float* live_depth, const float* live_normals,
                                          const float* live_intensity, const float* pred_depth,
                                          const float* pred_normals, const float* pred_intensity, double* twist_inout,
                                          double* records, void* scratch, float* residuals_out,
                                          float* intensity_residuals_out, float* weights_out,
                                          const lsf_icp_pyramid_robust_params* params, void* stream) {
    (void)hipGetLastError();
    if (!live_depth || !live_normals || !pred_depth || !pred_normals || !twist_inout || !scratch || !params ||
        !robust_term(params, live_intensity, pred_intensity, intensity_residuals_out))
        return LSF_ERR_BAD_ARGUMENT;
    return run_pyramid(settings_of(params, weights_out),
                       {live_depth, live_normals, live_intensity, pred_depth, pred_normals, pred_intensity,
                        twist_inout, records, scratch, residuals_out, intensity_residuals_out},
                       LSF_ICP_PYRAMID_ROBUST_SCRATCH_BYTES, stream);
}
