// What the Gauss-Newton trackers over a live depth image share (lsf_icp.hip: projective point-to-plane ICP against the
// ray-cast prediction; lsf_point_sdf.hip: point-to-SDF against the model itself): the layout of the per-block sums and
// of the record, the strided and the pyramid source and their levels, the robust weight, a term's rows (add_rows), the
// composed update, the launch-boundary prologue, the finishing kernel, the launch schedule, the select over (colour
// term, loss) and the host checks.  Each tracker keeps its own per-pixel body.
// Everything here has internal linkage, as it had inside lsf_icp.hip before it moved: the kernels of that file
// compile to the code they compiled to there (profiles/point_sdf_cost.md).
#pragma once

#include <cstddef>
#include <initializer_list>

#include "lsf_device.h"
#include "lsf_rigid_solve.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kTile = 16;  // a workgroup covers 16 x 16 strided pixels
constexpr int kSub = 8;    // a wave's block is kSub x kSub of them
constexpr int kSums = 29;  // A's upper triangle (21, row by row), b (6), energy, count
constexpr int kRobustSums = 3;     // a robust source: its base's, then sum w, sum w_I and the geometric outliers
constexpr int kMaxBlocks = LSF_ICP_MAX_BLOCKS;
constexpr int kRecord = LSF_ICP_RECORD_DOUBLES;
constexpr int kDelta = 0, kTwist = 6, kEnergy = 12, kA = 13, kB = 49, kSkipped = 55, kCount = 56, kLevel = 57,
              kRejected = 58, kPhotoCount = 59, kPhotoEnergy = 60, kWeightSum = 61, kPhotoWeightSum = 62,
              kOutliers = 63;
static_assert(kSub * kSub == kWave && (kTile / kSub) * (kTile / kSub) * kWave == kBlock, "4 waves of 8 x 8 pixels");
static_assert(kMaxBlocks <= kBlock, "the prologue gives every partial one thread");
static_assert(kOutliers < kRecord && kRejected < kRecord && kB == kA + 36 && kSkipped == kB + 6, "the record holds every field");

// where a source keeps its sums: kSums, then the gate's rejections (a pyramid source; the point-to-SDF source keeps
// its pixels without a valid sample there), the photometric pairs and sum r_I^2 (a photometric one), and sum w, sum w_I
// and the geometric outliers (a robust one)
template <bool PYRAMID, bool PHOTO, bool ROBUST>
struct Sums {
    static constexpr bool kPyramid = PYRAMID, kPhoto = PHOTO, kRobust = ROBUST;
    static constexpr int kPhotoAt = kSums + (PYRAMID ? 1 : 0), kRobustAt = kPhotoAt + (PHOTO ? 2 : 0),
                         K = kRobustAt + (ROBUST ? kRobustSums : 0);
};

struct IcpDev {
    double fx, fy, cx, cy, ratio, max_distance;
    double twist_p[6];  // the prediction's camera: live_extrinsic(twist_p), the ray-cast's
    int height, width;
};

// the pixels (i, j), i < ni, j < nj, of one launch's level and their 16 x 16 tiles
struct Grid {
    int ni, nj, tiles_x, tiles;
};

Grid grid_of(int ni, int nj) {
    const int tiles_x = (ni + kTile - 1) / kTile;
    return {ni, nj, tiles_x, tiles_x * ((nj + kTile - 1) / kTile)};
}

// lsf_icp_run: pixel (i, j) is the live image's (stride i, stride j), its depth scaled by the ratio
template <typename DT>
struct StridedSource {
    using Layout = Sums<false, false, false>;
    static constexpr int K = Layout::K;
    static constexpr bool kGate = false, kPhoto = false, kRobust = false;
    using Live = DT;
    Grid grid;
    int stride;
    static constexpr long long offset = 0;  // of the level in the live buffers

    struct Pixel {
        int u, v;  // < width, height: ni = ceil(width / stride)
    };
    __device__ Pixel pixel(int i, int j) const { return {i * stride, j * stride}; }
    // the depth of a pixel in metres (it has one when it is > 0), and its vertex in camera coordinates
    __device__ double depth(const DT* __restrict__ live, const IcpDev& p, Pixel px) const {
        return (double)scaled_depth(live, (long long)px.v * p.width + px.u, p.ratio);
    }
    __device__ void vertex(const IcpDev& p, Pixel px, double d, double (&vx)[3]) const {
        vx[0] = d * (((double)px.u - p.cx) / p.fx);
        vx[1] = d * (((double)px.v - p.cy) / p.fy);
        vx[2] = d * 1.0;
    }
    // r at the pixel, NaN at the rest of its stride x stride cell
    __device__ void store(float* __restrict__ residuals, const IcpDev& p, Pixel px, float res) const {
        for (int y = px.v; y < min(px.v + stride, p.height); ++y)
            for (int x = px.u; x < min(px.u + stride, p.width); ++x)
                residuals[(long long)y * p.width + x] = (x == px.u && y == px.v) ? res : NAN;
    }
};

// lsf_icp_run_pyramid: every pixel of one pyramid level, float32 metres at live[j ni + i], normals beside them
template <bool GATE>
struct PyramidSource {
    using Layout = Sums<true, false, false>;
    static constexpr int K = Layout::K;
    static constexpr bool kGate = GATE, kPhoto = false, kRobust = false;
    using Live = float;
    double fx, fy, cx, cy, cos_max;
    long long offset;  // of the level in the live buffers: the launch passes their pointers advanced by it
    Grid grid;

    struct Pixel {
        int i, j;
        long long at;  // in the level's arrays
    };
    __device__ Pixel pixel(int i, int j) const { return {i, j, (long long)j * grid.ni + i}; }
    __device__ double depth(const float* __restrict__ live, const IcpDev&, Pixel px) const {
        return (double)live[px.at];
    }
    __device__ void vertex(const IcpDev&, Pixel px, double d, double (&vx)[3]) const {
        vx[0] = d * (((double)px.i - cx) / fx);
        vx[1] = d * (((double)px.j - cy) / fy);
        vx[2] = d * 1.0;
    }
    __device__ const float* normal(const float* __restrict__ normals, Pixel px) const { return normals + px.at * 3; }
    __device__ void store(float* __restrict__ residuals, const IcpDev&, Pixel px, float res) const {
        residuals[px.at] = res;
    }
};

// lsf_icp_run_robust and lsf_icp_run_pyramid_robust: BASE's pixels, pairs and gates; a pair's rows are scaled by the
// weight of its own residual, w from r and scale, w_I from the unscaled r_I and intensity_scale.  The loss is the same
// for every lane of a launch, so the select is wave-uniform
template <typename BASE>
struct RobustSource : BASE {
    using Layout = Sums<BASE::Layout::kPyramid, BASE::kPhoto, true>;
    static constexpr int K = Layout::K;
    static constexpr bool kRobust = true;
    int loss;  // LSF_ICP_LOSS_*
    double scale, intensity_scale;
    float* weights;  // w of the launch, laid out like the residuals, or NULL: launch_schedule keeps it for the last iteration

    // the weight of the residual r at the scale s (> 0, inf allowed), and whether the pair is an outlier
    __device__ double weight(double r, double s, bool& outlier) const {
        const double a = fabs(r);
        if (loss == LSF_ICP_LOSS_HUBER) {
            outlier = a > s;
            return a <= s ? 1.0 : s / a;
        }
        const double t = r / s;
        const double u = 1.0 - t * t;
        outlier = a >= s;
        return a < s ? u * u : 0.0;
    }
};

// the rows of one term, J and r with the weight w (1 without a loss), into A's upper triangle, b
template <bool ROBUST, int K>
__device__ __forceinline__ void add_rows(const double (&J)[6], double r, double w, double (&acc)[K]) {
    int n = 0;
    if constexpr (ROBUST) {
        double wJ[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) wJ[a] = w * J[a];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[n++] += wJ[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] -= wJ[a] * r;
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[n++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] -= J[a] * r;
    }
}

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
// L (a Sums): a pyramid source's also writes the gate's rejections to record slot kRejected, a photometric one's the
// photometric pairs and energy to kPhotoCount and kPhotoEnergy, a robust one's sum w, sum w_I and the outliers to
// kWeightSum, kPhotoWeightSum and kOutliers; the slots a source does not have are 0.
template <typename L>
__device__ __forceinline__ void icp_prologue(int k, int prev_blocks, int prev_level, double* __restrict__ twist_io,
                                             double* __restrict__ records, const double* __restrict__ scratch,
                                             double (*red)[L::K], double* tw, double* twist_final) {
    if (k == 0) {
        if (threadIdx.x == 0)
            for (int i = 0; i < 6; ++i) tw[i] = twist_io[i];
        __syncthreads();
        return;
    }
    constexpr int K = L::K;
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
            for (int i = kLevel + 1; i < kRecord; ++i) r[i] = 0.0;
            if constexpr (L::kPyramid) r[kRejected] = v[kSums];
            if constexpr (L::kPhoto) {
                r[kPhotoCount] = v[L::kPhotoAt];
                r[kPhotoEnergy] = v[L::kPhotoAt + 1];
            }
            if constexpr (L::kRobust) {
                r[kWeightSum] = v[L::kRobustAt];
                r[kPhotoWeightSum] = v[L::kRobustAt + 1];
                r[kOutliers] = v[L::kRobustAt + 2];
            }
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

// the prologue alone, one block: the last iteration's record and the final twist.  L: the sums of the run's source
template <typename L>
__global__ __launch_bounds__(kBlock) void icp_finish_kernel(double* __restrict__ twist_io, double* __restrict__ records,
                                                            const double* __restrict__ scratch, int k, int prev_blocks,
                                                            int prev_level) {
    __shared__ double red[kBlock / kWave][L::K];
    __shared__ double tw[6];
    icp_prologue<L>(k, prev_blocks, prev_level, twist_io, records, scratch, red, tw, twist_io);
}

// the schedule: levels coarse first, iterations[l] launches over source_of(l), each by launch(src, blocks, k,
// prev_blocks, prev_level, last) -- last: launch total - 1, the one that keeps the residuals; a robust source keeps its
// weight image for that launch only --, then the finishing launch
template <typename SourceOf, typename Launch>
int launch_schedule(int levels, const int32_t* iterations, int total, double* twist, double* records, double* scratch,
                    hipStream_t stream, SourceOf source_of, Launch launch) {
    using SRC = decltype(source_of(0));
    int k = 0, prev_blocks = 0, prev_level = 0;
    for (int l = 0; l < levels; ++l) {
        const SRC level = source_of(l);
        const int blocks = level.grid.tiles < kMaxBlocks ? level.grid.tiles : kMaxBlocks;
        for (int it = 0; it < iterations[l]; ++it, ++k) {
            SRC src = level;
            if constexpr (SRC::kRobust)
                if (k != total - 1) src.weights = nullptr;
            launch(src, blocks, k, prev_blocks, prev_level, k == total - 1);
            if (int e = launch_status()) return e;
            prev_blocks = blocks;
            prev_level = l;
        }
    }
    hipLaunchKernelGGL(icp_finish_kernel<typename SRC::Layout>, dim3(1), dim3(kBlock), 0, stream, twist, records,
                       scratch, total, prev_blocks, prev_level);
    return launch_status();
}

// a strided level of a height x width live image: the pixels (stride i, stride j)
template <typename DT>
StridedSource<DT> strided_level(int height, int width, int stride) {
    return {grid_of((width + stride - 1) / stride, (height + stride - 1) / stride), stride};
}

// the source of iterations entry l of a pyramid run of `levels` tracked levels over a height x width level 0:
// lsf_depth_pyramid's layout and level intrinsics
template <bool GATE>
PyramidSource<GATE> pyramid_level(double fx, double fy, double cx, double cy, double cos_max, int height, int width,
                                  int levels, int l) {
    PyramidSource<GATE> src = {fx, fy, cx, cy, cos_max, 0, {}};
    const int level = levels - 1 - l;
    for (int c = 0; c < level; ++c) {
        src.offset += (long long)(height >> c) * (width >> c);
        src.fx = src.fx / 2.0;
        src.fy = src.fy / 2.0;
        src.cx = (src.cx - 0.5) / 2.0;
        src.cy = (src.cy - 0.5) / 2.0;
    }
    src.grid = grid_of(width >> level, height >> level);
    return src;
}

// the pixels of a pyramid's buffer
size_t pyramid_pixels(int height, int width, int pyramid_levels) {
    size_t n = 0;
    for (int l = 0; l < pyramid_levels; ++l) n += (size_t)(height >> l) * (width >> l);
    return n;
}

// the pixels of the last iteration's pyramid level: the extents of the residual images
size_t last_level_pixels(int height, int width, int levels, const int32_t* iterations) {
    int last = 0;
    for (int l = 0; l < levels; ++l)
        if (iterations[l] > 0) last = levels - 1 - l;
    return (size_t)(height >> last) * (width >> last);
}

// the optional loss of a run: loss 0 is none, and then the rest is not read
struct Loss {
    int loss;  // 0 or LSF_ICP_LOSS_*
    double scale, intensity_scale;
    float* weights_out;
};

// the run over level(l) with the optional colour term (coloured(base): the file's colour source over a level) and the
// optional loss: one of four sources goes to launch(source_of), the file's launch_run over its own run
template <typename Launch, typename LevelOf, typename Coloured>
int launch_selected(bool term, const Loss& w, Launch launch, LevelOf level, Coloured coloured) {
    auto robust = [&](auto base) {
        return RobustSource<decltype(base)>{base, w.loss, w.scale, w.intensity_scale, w.weights_out};
    };
    if (!term && !w.loss) return launch(level);
    if (!term) return launch([&](int l) { return robust(level(l)); });
    if (!w.loss) return launch([&](int l) { return coloured(level(l)); });
    return launch([&](int l) { return robust(coloured(level(l))); });
}

// sum(iterations), or -1 when an entry is negative, the records would not fit an int index, or there are none to
// write them to
long long iteration_total(const int32_t* iterations, int levels, const double* records) {
    long long total = 0;
    for (int l = 0; l < levels; ++l) {
        if (iterations[l] < 0) return -1;
        total += iterations[l];
    }
    return total > 0x7fffffffll / kRecord || (total > 0 && !records) ? -1 : total;
}

struct Buffer {
    const void* at;  // may be NULL: aliases nothing
    size_t bytes;
};

// an output overlaps an input or another output
bool aliased(std::initializer_list<Buffer> outs, std::initializer_list<Buffer> ins) {
    auto overlaps = [](const Buffer& a, const Buffer& b) {
        const uintptr_t x = (uintptr_t)a.at, y = (uintptr_t)b.at;
        return a.at && b.at && x < y + b.bytes && y < x + a.bytes;
    };
    for (const Buffer* o = outs.begin(); o != outs.end(); ++o) {
        for (const Buffer& in : ins)
            if (overlaps(*o, in)) return true;
        for (const Buffer* other = o + 1; other != outs.end(); ++other)
            if (overlaps(*o, *other)) return true;
    }
    return false;
}

}  // namespace
