// Fusion of aligned frames into a canonical TSDF volume (include/lsf_hip.h, lsf_fusion_*): the model update of
// KillingFusion / SobolevFusion, which the reference does not have; the rule is this project's (INTEGRATION.md
// section 3, "Fusion"; tests/fusion_restatement.py restates it).  One kernel, two live sources, one update:
//   VOLUME  the live value of a voxel is read from a given float32 field (flat index, 16-byte accesses per lane)
//   DEPTH   the live value is generated from a depth image under a twist by the rigid 3-D tracker's own code
//           (live_extrinsic + typed_tsdf_voxel, lsf_tsdf_typed.h, with its host setup and dispatch) and fused in the
//           same pass; no live volume is written
// Every lane takes four consecutive voxels per step of a grid-stride loop; the grid depends on the voxel count alone,
// so both sources visit the voxels in one order and sum the record identically.  Per-workgroup partials go to
// scratch; a finishing one-workgroup launch combines them in a fixed order (the sums by the trackers' butterfly,
// wave_sum_xor in lsf_rigid_solve.h): no atomics, reruns are bit-identical.
// -ffp-contract=off keeps W t + w l two roundings and an add, as numpy computes it.
// lsf_fusion_integrate_depth_weighted is the DEPTH kernel with the weighted rule ("Weighted
// fusion and carving"; tests/fusion_weighted_restatement.py): the same four voxels per lane, 16-byte accesses, grid and
// finishing launch, with the pixel a voxel projects to (typed_tsdf_sample) selecting its weight from a float32 image,
// +1 fused in the seen free space in front of the band, and six partials per workgroup instead of four.
// lsf_fusion_integrate_depth_colour is that kernel again with a colour volume beside the model (INTEGRATION.md section 3,
// "Colour fusion"; tests/colour_restatement.py): one float32 (R, G, B, Wc) record per voxel, loaded and stored in one
// 16-byte access each and only where the voxel lies inside the colour band, three byte reads of the colour image at the
// voxel's pixel, and eight partials per workgroup.  The geometry code is fuse_voxel_weighted itself.
// lsf_fusion_integrate_depth_warped is the non-rigid step's fusion ("Warped depth fusion";
// tests/warped_fusion_restatement.py): a voxel observes the frame at its point displaced by a warp field, float32
// (Z, Y, X, 3) interleaved -- 12 floats per four-voxel step, three 16-byte loads -- and fuse_voxel_weighted and
// colour_voxel run unchanged on what that point sees (typed_tsdf_sample_at); nine partials per workgroup.
#include "lsf_device.h"
#include "lsf_rigid_solve.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kParts = 4;   // fused, first_seen, sum |t1 - t|, max |t1 - t|
constexpr int kWParts = 6;  // the weighted rule: those, carved, weight_rejected
constexpr int kCParts = 8;  // with colour: those, coloured, first_coloured
constexpr int kXParts = 9;  // through a warp field: those, warp_rejected
constexpr int kMaxPart = 3; // the one partial that is a maximum; every other is a sum
constexpr int kMaxBlocks = LSF_FUSION_MAX_BLOCKS;
constexpr int kRec = LSF_FUSION_RECORD_DOUBLES;
static_assert(kRec >= kWParts && kRec >= kCParts, "the record holds the results of every rule");
static_assert(LSF_FUSION_SCRATCH_BYTES == kMaxBlocks * kParts * 8, "a workgroup's partials");
static_assert(LSF_FUSION_WEIGHTED_SCRATCH_BYTES == kMaxBlocks * kWParts * 8, "a workgroup's partials");
static_assert(LSF_FUSION_COLOUR_SCRATCH_BYTES == kMaxBlocks * kCParts * 8, "a workgroup's partials");
static_assert(LSF_FUSION_WARPED_SCRATCH_BYTES == kMaxBlocks * kXParts * 8, "a workgroup's partials");
static_assert(LSF_FUSION_WARPED_RECORD_DOUBLES == kXParts, "the warped record is its partials");

enum Source { VOLUME = 0, DEPTH = 1 };

struct FusionDev {
    TypedTsdf t;        // DEPTH
    double twist[6];    // DEPTH
    long long n;        // voxels
    long long groups;   // n / 4: the four-voxel steps; the n % 4 voxels after them are the tail
    int ny, nx;         // DEPTH: the flat index's y and x extents
    float w, max_weight;
    int aligned;        // every buffer read or written with 16-byte accesses is 16-byte aligned
    int nblocks;        // the grid: min(ceil(groups / kBlock), kMaxBlocks), at least 1; the number of partials
};

struct Acc {
    int fused, first;
    double sum;
    float max;
};

struct WeightedAcc {
    Acc a;
    int carved, rejected;
};

struct ColourAcc {
    WeightedAcc w;
    int coloured, first;
};

// the colour side of a call: the volume of (R, G, B, Wc) records, the uint8 (R, G, B) image, the band
struct ColourDev {
    float4* __restrict__ volume;
    const unsigned char* __restrict__ image;
    float band;
};

// the rule at one voxel; true when the voxel was observed (and its tsdf and weight may have changed)
__device__ inline bool fuse_voxel(float l, float& t, float& W, const FusionDev& p, Acc& a) {
    if (!(l > -1.0f && l < 1.0f)) return false;  // +-1 and NaN are not fused
    const float W1 = W + p.w;
    const float t1 = (W * t + p.w * l) / W1;
    const float d = fabsf(t1 - t);
    a.fused += 1;
    a.first += W == 0.0f ? 1 : 0;
    a.sum += (double)d;
    a.max = d > a.max ? d : a.max;
    t = t1;
    W = W1 > p.max_weight ? p.max_weight : W1;
    return true;
}

// the weighted rule at one voxel.  s: what the voxel sees (typed_tsdf_sample); in band it is fused as fuse_voxel does,
// at exactly +1 with a valid pixel it is carved (fused with l = 1) when carve is set; the weight is w times the pixel's
// (one float32 multiply), and a weight that is not finite and > 0 leaves the voxel alone and is counted
__device__ inline bool fuse_voxel_weighted(const TsdfSample& s, const float* __restrict__ pixel_weight, bool carve,
                                           float& t, float& W, const FusionDev& p, WeightedAcc& acc) {
    if (!s.valid) return false;
    const float l = s.value;
    const bool band = l > -1.0f && l < 1.0f;
    if (!band && !(carve && l == 1.0f)) return false;
    const float w = pixel_weight ? p.w * pixel_weight[s.pixel] : p.w;
    if (!(w > 0.0f) || isinf(w)) {
        acc.rejected += 1;
        return false;
    }
    const float W1 = W + w;
    const float t1 = (W * t + w * l) / W1;
    const float d = fabsf(t1 - t);
    acc.a.fused += band ? 1 : 0;
    acc.carved += band ? 0 : 1;
    acc.a.first += W == 0.0f ? 1 : 0;
    acc.a.sum += (double)d;
    acc.a.max = d > acc.a.max ? d : acc.a.max;
    t = t1;
    W = W1 > p.max_weight ? p.max_weight : W1;
    return true;
}

// the colour rule at voxel i, after fuse_voxel_weighted has updated it (so its pixel is valid and its weight usable):
// inside the colour band -- which lies in (-1, 1), so a carved voxel never is -- its record is averaged with the pixel's
// colour under the same weight, one 16-byte load and one 16-byte store; outside, colour memory is not touched
__device__ inline void colour_voxel(const TsdfSample& s, const float* __restrict__ pixel_weight, const ColourDev& c,
                                    long long i, const FusionDev& p, ColourAcc& acc) {
    const float l = s.value;
    if (!(l > -c.band && l < c.band)) return;
    const float w = pixel_weight ? p.w * pixel_weight[s.pixel] : p.w;
    const unsigned char* px = c.image + s.pixel * 3;
    const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
    float4 q = c.volume[i];
    const float Wc = q.w, Wc1 = Wc + w;
    q.x = (Wc * q.x + w * r) / Wc1;
    q.y = (Wc * q.y + w * g) / Wc1;
    q.z = (Wc * q.z + w * b) / Wc1;
    q.w = Wc1 > p.max_weight ? p.max_weight : Wc1;
    c.volume[i] = q;
    acc.coloured += 1;
    acc.first += Wc == 0.0f ? 1 : 0;
}

__device__ inline void load4(const float* __restrict__ f, long long i, float (&v)[4], bool aligned) {
    if (aligned) {
        const float4 q = *reinterpret_cast<const float4*>(f + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = f[i + k];
    }
}

__device__ inline void store4(float* __restrict__ f, long long i, const float (&v)[4], bool aligned) {
    if (aligned) {
        *reinterpret_cast<float4*>(f + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) f[i + k] = v[k];
    }
}

// what voxel i (flat [z][y][x] index) sees under extrinsic e: lsf_rigid3d_gradient's generation
template <typename DT, typename PT>
__device__ inline TsdfSample depth_sample(const DT* __restrict__ depth, const FusionDev& p, const double* e,
                                          long long i) {
    const long long row = i / p.nx;
    const int x = (int)(i - row * p.nx);
    const int z = (int)(row / p.ny);
    const int y = (int)(row - (long long)z * p.ny);
    return typed_tsdf_sample<3, double, PT, DT>(depth, p.t, e, x, y, z);
}

// its live value alone
template <typename DT, typename PT>
__device__ inline float depth_voxel(const DT* __restrict__ depth, const FusionDev& p, const double* e, long long i) {
    return depth_sample<DT, PT>(depth, p, e, i).value;
}

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}

// the block's totals of v[] (counts and sum added, max taken) in a fixed order; they land in thread 0's v[]
template <int N>
__device__ inline void block_combine(double (&v)[N], double (*red)[N]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = c == kMaxPart ? (double)wave_max((float)v[c]) : wave_sum_xor(v[c]);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) red[wave][c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < kBlock / kWave; ++q) {
#pragma unroll
            for (int c = 0; c < N; ++c)
                if (c == kMaxPart) v[c] = red[q][c] > v[c] ? red[q][c] : v[c];
                else v[c] += red[q][c];
        }
}

template <int SOURCE, typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void fusion_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                        const float* __restrict__ live,
                                                        const DT* __restrict__ depth, double* __restrict__ scratch,
                                                        FusionDev p) {
    __shared__ double e[12];
    __shared__ double red[kBlock / kWave][kParts];
    if (SOURCE == DEPTH) {
        if (threadIdx.x == 0) live_extrinsic(p.twist, e);
        __syncthreads();
    }
    const bool aligned = p.aligned != 0;
    Acc a = {0, 0, 0.0, 0.0f};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += stride) {
        const long long i = g * 4;
        float l[4], t[4], W[4];
        if (SOURCE == VOLUME) {
            load4(live, i, l, aligned);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) l[k] = depth_voxel<DT, PT>(depth, p, e, i + k);
        }
        load4(tsdf, i, t, aligned);
        load4(weight, i, W, aligned);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) any = fuse_voxel(l[k], t[k], W[k], p, a) || any;
        if (any) {  // a step without an observed voxel stores nothing; the stored values would equal the loaded ones
            store4(tsdf, i, t, aligned);
            store4(weight, i, W, aligned);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the tail, after this lane's steps
        for (long long i = p.groups * 4; i < p.n; ++i) {
            const float l = SOURCE == VOLUME ? live[i] : depth_voxel<DT, PT>(depth, p, e, i);
            float t = tsdf[i], W = weight[i];
            if (fuse_voxel(l, t, W, p, a)) {
                tsdf[i] = t;
                weight[i] = W;
            }
        }
    double v[kParts] = {(double)a.fused, (double)a.first, a.sum, (double)a.max};
    block_combine(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < kParts; ++c) scratch[(size_t)blockIdx.x * kParts + c] = v[c];
}

// the weighted rule on a depth image: fusion_kernel<DEPTH>'s walk, stores and partials with fuse_voxel_weighted
template <typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void fusion_weighted_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                 const DT* __restrict__ depth,
                                                                 const float* __restrict__ pixel_weight,
                                                                 double* __restrict__ scratch, FusionDev p, int carve) {
    __shared__ double e[12];
    __shared__ double red[kBlock / kWave][kWParts];
    if (threadIdx.x == 0) live_extrinsic(p.twist, e);
    __syncthreads();
    const bool aligned = p.aligned != 0, carving = carve != 0;
    WeightedAcc a = {{0, 0, 0.0, 0.0f}, 0, 0};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += stride) {
        const long long i = g * 4;
        TsdfSample s[4];
        float t[4], W[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = depth_sample<DT, PT>(depth, p, e, i + k);
        load4(tsdf, i, t, aligned);
        load4(weight, i, W, aligned);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) any = fuse_voxel_weighted(s[k], pixel_weight, carving, t[k], W[k], p, a) || any;
        if (any) {  // a step without an updated voxel stores nothing
            store4(tsdf, i, t, aligned);
            store4(weight, i, W, aligned);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the tail, after this lane's steps
        for (long long i = p.groups * 4; i < p.n; ++i) {
            float t = tsdf[i], W = weight[i];
            if (fuse_voxel_weighted(depth_sample<DT, PT>(depth, p, e, i), pixel_weight, carving, t, W, p, a)) {
                tsdf[i] = t;
                weight[i] = W;
            }
        }
    double v[kWParts] = {(double)a.a.fused, (double)a.a.first, a.a.sum, (double)a.a.max, (double)a.carved,
                         (double)a.rejected};
    block_combine(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < kWParts; ++c) scratch[(size_t)blockIdx.x * kWParts + c] = v[c];
}

// the weighted rule with colour: fusion_weighted_kernel's walk, stores and partials, and colour_voxel at every updated voxel
template <typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void fusion_colour_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                               const DT* __restrict__ depth,
                                                               const float* __restrict__ pixel_weight,
                                                               double* __restrict__ scratch, FusionDev p, int carve,
                                                               ColourDev c) {
    __shared__ double e[12];
    __shared__ double red[kBlock / kWave][kCParts];
    if (threadIdx.x == 0) live_extrinsic(p.twist, e);
    __syncthreads();
    const bool aligned = p.aligned != 0, carving = carve != 0;
    ColourAcc a = {{{0, 0, 0.0, 0.0f}, 0, 0}, 0, 0};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += stride) {
        const long long i = g * 4;
        TsdfSample s[4];
        float t[4], W[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = depth_sample<DT, PT>(depth, p, e, i + k);
        load4(tsdf, i, t, aligned);
        load4(weight, i, W, aligned);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (fuse_voxel_weighted(s[k], pixel_weight, carving, t[k], W[k], p, a.w)) {
                any = true;
                colour_voxel(s[k], pixel_weight, c, i + k, p, a);
            }
        if (any) {  // a step without an updated voxel stores nothing
            store4(tsdf, i, t, aligned);
            store4(weight, i, W, aligned);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the tail, after this lane's steps
        for (long long i = p.groups * 4; i < p.n; ++i) {
            float t = tsdf[i], W = weight[i];
            const TsdfSample s = depth_sample<DT, PT>(depth, p, e, i);
            if (fuse_voxel_weighted(s, pixel_weight, carving, t, W, p, a.w)) {
                tsdf[i] = t;
                weight[i] = W;
                colour_voxel(s, pixel_weight, c, i, p, a);
            }
        }
    double v[kCParts] = {(double)a.w.a.fused, (double)a.w.a.first,  a.w.a.sum,          (double)a.w.a.max,
                         (double)a.w.carved,  (double)a.w.rejected, (double)a.coloured, (double)a.first};
    block_combine(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c8 = 0; c8 < kCParts; ++c8) scratch[(size_t)blockIdx.x * kCParts + c8] = v[c8];
}

// the twelve warp floats of the four voxels from i on: three 16-byte loads, or scalar ones off alignment
__device__ inline void load_warp4(const float* __restrict__ warp, long long i, float (&v)[12], bool aligned) {
    const float* f = warp + i * 3;
    if (aligned) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 q = reinterpret_cast<const float4*>(f)[k];
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = f[k];
    }
}

// what voxel i sees at its point displaced by psi = (px, py, pz) voxels: depth_sample with one float64 add in front of
// the voxel point's expression, so psi = +-0 gives depth_sample's bits.  A psi that is not finite sees nothing and is
// counted
template <typename DT, typename PT>
__device__ inline TsdfSample warped_sample(const DT* __restrict__ depth, const FusionDev& p, const double* e,
                                           long long i, float px, float py, float pz, int& rejected) {
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) {
        rejected += 1;
        return {p.t.default_value, -1, false};
    }
    const long long row = i / p.nx;
    const int x = (int)(i - row * p.nx);
    const int z = (int)(row / p.ny);
    const int y = (int)(row - (long long)z * p.ny);
    const float xv = (float)((((double)x + (double)px) + p.t.off[0]) * p.t.voxel_size);
    const float yv = (float)((((double)y + (double)py) + p.t.off[1]) * p.t.voxel_size);
    const float zv = (float)((((double)z + (double)pz) + p.t.off[2]) * p.t.voxel_size);
    return typed_tsdf_sample_at<3, double, PT, DT>(depth, p.t, e, xv, yv, zv);
}

// the weighted rule (and colour, when c.volume is given) at the warped point of every voxel: fusion_colour_kernel's
// walk, stores and partials
template <typename DT, typename PT>
__global__ __launch_bounds__(kBlock) void fusion_warped_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                               const float* __restrict__ warp,
                                                               const DT* __restrict__ depth,
                                                               const float* __restrict__ pixel_weight,
                                                               double* __restrict__ scratch, FusionDev p, int carve,
                                                               ColourDev c, int warp_aligned) {
    __shared__ double e[12];
    __shared__ double red[kBlock / kWave][kXParts];
    if (threadIdx.x == 0) live_extrinsic(p.twist, e);
    __syncthreads();
    const bool aligned = p.aligned != 0, carving = carve != 0, psi_aligned = warp_aligned != 0;
    const bool colouring = c.volume != nullptr;
    ColourAcc a = {{{0, 0, 0.0, 0.0f}, 0, 0}, 0, 0};
    int rejected = 0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += stride) {
        const long long i = g * 4;
        TsdfSample s[4];
        float psi[12], t[4], W[4];
        load_warp4(warp, i, psi, psi_aligned);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            s[k] = warped_sample<DT, PT>(depth, p, e, i + k, psi[3 * k], psi[3 * k + 1], psi[3 * k + 2], rejected);
        load4(tsdf, i, t, aligned);
        load4(weight, i, W, aligned);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (fuse_voxel_weighted(s[k], pixel_weight, carving, t[k], W[k], p, a.w)) {
                any = true;
                if (colouring) colour_voxel(s[k], pixel_weight, c, i + k, p, a);
            }
        if (any) {  // a step without an updated voxel stores nothing
            store4(tsdf, i, t, aligned);
            store4(weight, i, W, aligned);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the tail, after this lane's steps
        for (long long i = p.groups * 4; i < p.n; ++i) {
            float t = tsdf[i], W = weight[i];
            const float* f = warp + i * 3;
            const TsdfSample s = warped_sample<DT, PT>(depth, p, e, i, f[0], f[1], f[2], rejected);
            if (fuse_voxel_weighted(s, pixel_weight, carving, t, W, p, a.w)) {
                tsdf[i] = t;
                weight[i] = W;
                if (colouring) colour_voxel(s, pixel_weight, c, i, p, a);
            }
        }
    double v[kXParts] = {(double)a.w.a.fused, (double)a.w.a.first,  a.w.a.sum,          (double)a.w.a.max,
                         (double)a.w.carved,  (double)a.w.rejected, (double)a.coloured, (double)a.first,
                         (double)rejected};
    block_combine(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c9 = 0; c9 < kXParts; ++c9) scratch[(size_t)blockIdx.x * kXParts + c9] = v[c9];
}

// one workgroup: lane q combines partials q, q + kBlock, ... in order, then the block in a fixed order
template <int N>
__global__ __launch_bounds__(kBlock) void fusion_finish_kernel(const double* __restrict__ scratch,
                                                               double* __restrict__ record, int nblocks) {
    __shared__ double red[kBlock / kWave][N];
    double v[N];
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = 0.0;
    for (int q = threadIdx.x; q < nblocks; q += kBlock) {
        const double* s = scratch + (size_t)q * N;
#pragma unroll
        for (int c = 0; c < N; ++c)
            if (c == kMaxPart) v[c] = s[c] > v[c] ? s[c] : v[c];
            else v[c] += s[c];
    }
    block_combine(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) record[c] = v[c];
        for (int c = N; c < kRec; ++c) record[c] = 0.0;
    }
}

bool aligned16(const void* ptr) { return ptr == nullptr || ((uintptr_t)ptr & 15) == 0; }

int convert(const lsf_fusion_params* params, FusionDev& p) {
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    if (params->depth < 1 || params->height < 1 || params->width < 1) return LSF_ERR_BAD_ARGUMENT;
    const float w = params->weight, cap = params->max_weight;
    if (!(w > 0.0f) || !std::isfinite(w) || !(cap > 0.0f)) return LSF_ERR_BAD_ARGUMENT;
    p.t = typed_tsdf(params->tsdf, params->array_offset, 0);
    for (int i = 0; i < 6; ++i) p.twist[i] = params->twist[i];
    p.n = (long long)params->depth * params->height * params->width;
    p.groups = p.n / 4;
    p.ny = params->height;
    p.nx = params->width;
    p.w = w;
    p.max_weight = cap;
    const long long want = (p.groups + kBlock - 1) / kBlock;
    p.nblocks = want < 1 ? 1 : (want > kMaxBlocks ? kMaxBlocks : (int)want);
    return 0;
}

template <int SOURCE, typename DT, typename PT>
int launch(float* tsdf, float* weight, const float* live, const void* depth, double* record, double* scratch,
           const FusionDev& p, hipStream_t s) {
    hipLaunchKernelGGL((fusion_kernel<SOURCE, DT, PT>), dim3(p.nblocks), dim3(kBlock), 0, s, tsdf, weight, live,
                       reinterpret_cast<const DT*>(depth), scratch, p);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(fusion_finish_kernel<kParts>, dim3(1), dim3(kBlock), 0, s, (const double*)scratch, record,
                       p.nblocks);
    return launch_status();
}

template <typename DT, typename PT>
int launch_weighted(float* tsdf, float* weight, const void* depth, const float* pixel_weight, double* record,
                    double* scratch, const FusionDev& p, int carve, hipStream_t s) {
    hipLaunchKernelGGL((fusion_weighted_kernel<DT, PT>), dim3(p.nblocks), dim3(kBlock), 0, s, tsdf, weight,
                       reinterpret_cast<const DT*>(depth), pixel_weight, scratch, p, carve);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(fusion_finish_kernel<kWParts>, dim3(1), dim3(kBlock), 0, s, (const double*)scratch, record,
                       p.nblocks);
    return launch_status();
}

template <typename DT, typename PT>
int launch_colour(float* tsdf, float* weight, const void* depth, const float* pixel_weight, double* record,
                  double* scratch, const FusionDev& p, int carve, const ColourDev& c, hipStream_t s) {
    hipLaunchKernelGGL((fusion_colour_kernel<DT, PT>), dim3(p.nblocks), dim3(kBlock), 0, s, tsdf, weight,
                       reinterpret_cast<const DT*>(depth), pixel_weight, scratch, p, carve, c);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(fusion_finish_kernel<kCParts>, dim3(1), dim3(kBlock), 0, s, (const double*)scratch, record,
                       p.nblocks);
    return launch_status();
}

template <typename DT, typename PT>
int launch_warped(float* tsdf, float* weight, const float* warp, const void* depth, const float* pixel_weight,
                  double* record, double* scratch, const FusionDev& p, int carve, const ColourDev& c, int warp_aligned,
                  hipStream_t s) {
    hipLaunchKernelGGL((fusion_warped_kernel<DT, PT>), dim3(p.nblocks), dim3(kBlock), 0, s, tsdf, weight, warp,
                       reinterpret_cast<const DT*>(depth), pixel_weight, scratch, p, carve, c, warp_aligned);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(fusion_finish_kernel<kXParts>, dim3(1), dim3(kBlock), 0, s, (const double*)scratch, record,
                       p.nblocks);
    return launch_status();
}

int check_buffers(const float* tsdf, const float* weight, const void* source, const double* record,
                  const void* scratch) {
    if (!tsdf || !weight || !source || !record || !scratch) return LSF_ERR_BAD_ARGUMENT;
    if ((const void*)tsdf == (const void*)weight || source == (const void*)tsdf || source == (const void*)weight)
        return LSF_ERR_BAD_ARGUMENT;
    return 0;
}

}  // namespace

extern "C" int lsf_fusion_integrate_volume(float* tsdf, float* weight, const float* live, double* record,
                                           void* scratch, const lsf_fusion_params* params, void* stream) {
    (void)hipGetLastError();
    if (int e = check_buffers(tsdf, weight, live, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(params, p)) return e;
    p.aligned = aligned16(tsdf) && aligned16(weight) && aligned16(live);
    return launch<VOLUME, float, double>(tsdf, weight, live, nullptr, record, reinterpret_cast<double*>(scratch), p,
                                         as_stream(stream));
}

extern "C" int lsf_fusion_integrate_depth(float* tsdf, float* weight, const void* depth_image, double* record,
                                          void* scratch, const lsf_fusion_params* params, void* stream) {
    (void)hipGetLastError();
    if (int e = check_buffers(tsdf, weight, depth_image, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(params, p)) return e;
    if (!depth_dtype_ok(params->depth_dtype) || !typed_tsdf_ok(params->tsdf, false, true))
        return LSF_ERR_BAD_ARGUMENT;
    p.aligned = aligned16(tsdf) && aligned16(weight);
    hipStream_t s = as_stream(stream);
    double* sc = reinterpret_cast<double*>(scratch);
    return dispatch_typed(params->depth_dtype, params->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch<DEPTH, decltype(dt), decltype(pt)>(tsdf, weight, nullptr, depth_image, record, sc, p, s);
    });
}

extern "C" int lsf_fusion_integrate_depth_weighted(float* tsdf, float* weight, const void* depth_image,
                                                   const float* pixel_weight, double* record, void* scratch,
                                                   const lsf_fusion_weighted_params* params, void* stream) {
    (void)hipGetLastError();
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_fusion_params* f = &params->fusion;
    if (int e = check_buffers(tsdf, weight, depth_image, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(f, p)) return e;
    if (!depth_dtype_ok(f->depth_dtype) || !typed_tsdf_ok(f->tsdf, false, true)) return LSF_ERR_BAD_ARGUMENT;
    if ((params->has_pixel_weight != 0) != (pixel_weight != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    if (pixel_weight) {
        const size_t image = (size_t)f->tsdf.image_width * f->tsdf.image_height * 4, model = (size_t)p.n * 4;
        if (overlaps(pixel_weight, image, tsdf, model) || overlaps(pixel_weight, image, weight, model))
            return LSF_ERR_BAD_ARGUMENT;
    }
    p.aligned = aligned16(tsdf) && aligned16(weight);
    hipStream_t s = as_stream(stream);
    double* sc = reinterpret_cast<double*>(scratch);
    const int carve = params->carve != 0;
    return dispatch_typed(f->depth_dtype, f->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch_weighted<decltype(dt), decltype(pt)>(tsdf, weight, depth_image, pixel_weight, record, sc, p,
                                                           carve, s);
    });
}

extern "C" int lsf_fusion_integrate_depth_colour(float* tsdf, float* weight, float* colour, const void* depth_image,
                                                 const float* pixel_weight, const uint8_t* colour_image,
                                                 double* record, void* scratch, const lsf_fusion_colour_params* params,
                                                 void* stream) {
    (void)hipGetLastError();
    if (!params || !colour || !colour_image) return LSF_ERR_BAD_ARGUMENT;
    const lsf_fusion_weighted_params* wp = &params->weighted;
    const lsf_fusion_params* f = &wp->fusion;
    if (int e = check_buffers(tsdf, weight, depth_image, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(f, p)) return e;
    if (!depth_dtype_ok(f->depth_dtype) || !typed_tsdf_ok(f->tsdf, false, true)) return LSF_ERR_BAD_ARGUMENT;
    if ((wp->has_pixel_weight != 0) != (pixel_weight != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    const float band = params->colour_band;
    if (!(band > 0.0f && band <= 1.0f)) return LSF_ERR_BAD_ARGUMENT;  // NaN fails
    if (((uintptr_t)colour & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t pixels = (size_t)f->tsdf.image_width * f->tsdf.image_height, model = (size_t)p.n * 4;
    const size_t depth_bytes = pixels * (f->depth_dtype == LSF_DEPTH_U16 ? 2 : (f->depth_dtype == LSF_DEPTH_F32 ? 4 : 8));
    const void* const buffers[6] = {tsdf, weight, colour, colour_image, pixel_weight, depth_image};
    const size_t bytes[6] = {model, model, model * 4, pixels * 3, pixels * 4, depth_bytes};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (overlaps(buffers[i], bytes[i], buffers[j], bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    p.aligned = aligned16(tsdf) && aligned16(weight);
    hipStream_t s = as_stream(stream);
    double* sc = reinterpret_cast<double*>(scratch);
    const int carve = wp->carve != 0;
    const ColourDev c{reinterpret_cast<float4*>(colour), colour_image, band};
    return dispatch_typed(f->depth_dtype, f->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch_colour<decltype(dt), decltype(pt)>(tsdf, weight, depth_image, pixel_weight, record, sc, p, carve,
                                                         c, s);
    });
}

extern "C" int lsf_fusion_integrate_depth_warped(float* tsdf, float* weight, float* colour, const float* warp,
                                                 const void* depth_image, const float* pixel_weight,
                                                 const uint8_t* colour_image, double* record, void* scratch,
                                                 const lsf_fusion_warped_params* params, void* stream) {
    (void)hipGetLastError();
    if (!params || !warp) return LSF_ERR_BAD_ARGUMENT;
    const lsf_fusion_weighted_params* wp = &params->colour.weighted;
    const lsf_fusion_params* f = &wp->fusion;
    if (int e = check_buffers(tsdf, weight, depth_image, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(f, p)) return e;
    if (!depth_dtype_ok(f->depth_dtype) || !typed_tsdf_ok(f->tsdf, false, true)) return LSF_ERR_BAD_ARGUMENT;
    if ((wp->has_pixel_weight != 0) != (pixel_weight != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    const bool has_colour = params->has_colour != 0;
    if (has_colour != (colour != nullptr) || has_colour != (colour_image != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    const float band = params->colour.colour_band;
    if (has_colour) {
        if (!(band > 0.0f && band <= 1.0f)) return LSF_ERR_BAD_ARGUMENT;  // NaN fails
        if (((uintptr_t)colour & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    }
    const size_t pixels = (size_t)f->tsdf.image_width * f->tsdf.image_height, model = (size_t)p.n * 4;
    const size_t depth_bytes = pixels * (f->depth_dtype == LSF_DEPTH_U16 ? 2 : (f->depth_dtype == LSF_DEPTH_F32 ? 4 : 8));
    const void* const buffers[7] = {tsdf, weight, colour, warp, depth_image, pixel_weight, colour_image};
    const size_t bytes[7] = {model, model, model * 4, model * 3, depth_bytes, pixels * 4, pixels * 3};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlaps(buffers[i], bytes[i], buffers[j], bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    p.aligned = aligned16(tsdf) && aligned16(weight);
    hipStream_t s = as_stream(stream);
    double* sc = reinterpret_cast<double*>(scratch);
    const int carve = wp->carve != 0, warp_aligned = aligned16(warp);
    const ColourDev c{reinterpret_cast<float4*>(colour), colour_image, has_colour ? band : 1.0f};
    return dispatch_typed(f->depth_dtype, f->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch_warped<decltype(dt), decltype(pt)>(tsdf, weight, warp, depth_image, pixel_weight, record, sc, p,
                                                         carve, c, warp_aligned, s);
    });
}
