// Fusion of aligned frames into a canonical TSDF volume (include/lsf_hip.h, lsf_fusion_*): the model update of
// KillingFusion / SobolevFusion, which the reference does not have; the rules are this project's (INTEGRATION.md
// section 3, "Fusion" and what follows it; tests/*_restatement.py restate them).
// One kernel, fusion_kernel<RULE>, walks the voxels for every entry point.  Every lane takes four consecutive voxels per
// step of a grid-stride loop: it asks the rule what the four observe, loads their tsdf and weight in one 16-byte access
// each (scalar ones off alignment), lets the rule fuse each in the order k = 0..3, and stores only when one of them
// changed.  The n % 4 voxels after the last step are the tail, taken by lane 0 of workgroup 0 after its own steps.  The
// grid depends on the voxel count alone, so every rule visits the voxels in one order and sums its record identically.
// Per-workgroup partials go to scratch; a finishing one-workgroup launch combines them in a fixed order (the sums by the
// trackers' butterfly, wave_sum_xor in lsf_rigid_solve.h): no atomics, reruns are bit-identical.
// -ffp-contract=off keeps W t + w l two roundings and an add, as numpy computes it.
// A rule says what a voxel observes and what is done with it:
//   VolumeRule    lsf_fusion_integrate_volume: the live value is read from a given float32 field (flat index)
//   DepthRule     lsf_fusion_integrate_depth: the live value is generated from a depth image under a twist by the rigid
//                 3-D tracker's own code (live_extrinsic + typed_tsdf_voxel, lsf_tsdf_typed.h, with its host setup and
//                 dispatch); no live volume is written.  Both fuse by fuse_voxel; four partials per workgroup
//   WeightedRule  the other three entry points: the voxel keeps the pixel it projects to (typed_tsdf_sample), which
//                 selects its weight from a float32 image, and +1 is fused in the seen free space in front of the band
//                 (fuse_voxel_weighted; six partials).  With WARP the voxel observes the frame at its point displaced by
//                 a warp field, float32 (Z, Y, X, 3) interleaved -- 12 floats per step, three 16-byte loads
//                 (typed_tsdf_sample_at; nine partials).  With COLOUR an updated voxel inside the colour band also
//                 averages its (R, G, B, Wc) record, one 16-byte load and store, with three byte reads of the colour
//                 image at its pixel (colour_voxel; eight partials); outside the band colour memory is not touched
#include <initializer_list>

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

// the weighted rule's: a counter that an instantiation never touches costs nothing
struct WarpedAcc {
    ColourAcc c;
    int rejected;
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

// ---- the rules.  A rule has N partials, an accumulator Acc, an observation Obs, kExtrinsic (whether e is needed), and
//   observe4(i, p, e, o, a)    what the four voxels from i on observe
//   observe(i, p, e, a)        what the tail voxel i observes
//   fuse(o, i, t, W, p, a)     the update of voxel i, which observed o; true when its tsdf and weight may have changed
//   parts(a, v)                the lane's partials

struct PlainRule {
    static constexpr int N = kParts;
    using Acc = ::Acc;
    using Obs = float;
    __device__ static bool fuse(float l, long long, float& t, float& W, const FusionDev& p, Acc& a) {
        return fuse_voxel(l, t, W, p, a);
    }
    __device__ static void parts(const Acc& a, double (&v)[N]) {
        v[0] = (double)a.fused; v[1] = (double)a.first; v[2] = a.sum; v[3] = (double)a.max;
    }
};

struct VolumeRule : PlainRule {
    static constexpr bool kExtrinsic = false;
    const float* __restrict__ live;
    __device__ void observe4(long long i, const FusionDev& p, const double*, float (&l)[4], Acc&) const {
        load4(live, i, l, p.aligned != 0);
    }
    __device__ float observe(long long i, const FusionDev&, const double*, Acc&) const { return live[i]; }
};

template <typename DT, typename PT>
struct DepthRule : PlainRule {
    static constexpr bool kExtrinsic = true;
    const DT* __restrict__ depth;
    __device__ void observe4(long long i, const FusionDev& p, const double* e, float (&l)[4], Acc&) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) l[k] = depth_voxel<DT, PT>(depth, p, e, i + k);
    }
    __device__ float observe(long long i, const FusionDev& p, const double* e, Acc&) const {
        return depth_voxel<DT, PT>(depth, p, e, i);
    }
};

enum Colour { NEVER = 0, ALWAYS = 1, IF_GIVEN = 2 };  // IF_GIVEN: when c.volume is given, one instantiation for both

template <typename DT, typename PT, bool WARP, int COLOUR, int PARTS>
struct WeightedRule {
    static_assert(PARTS == kWParts || PARTS == kCParts || PARTS == kXParts, "the three weighted records");
    static constexpr int N = PARTS;
    static constexpr bool kExtrinsic = true;
    using Acc = WarpedAcc;
    using Obs = TsdfSample;
    const DT* __restrict__ depth;
    const float* __restrict__ pixel_weight;
    const float* __restrict__ warp;  // WARP
    ColourDev c;                     // COLOUR
    int carve, warp_aligned;
    __device__ void observe4(long long i, const FusionDev& p, const double* e, TsdfSample (&s)[4], Acc& a) const {
        if constexpr (WARP) {
            float psi[12];
            load_warp4(warp, i, psi, warp_aligned != 0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                s[k] = warped_sample<DT, PT>(depth, p, e, i + k, psi[3 * k], psi[3 * k + 1], psi[3 * k + 2], a.rejected);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = depth_sample<DT, PT>(depth, p, e, i + k);
        }
    }
    __device__ TsdfSample observe(long long i, const FusionDev& p, const double* e, Acc& a) const {
        if constexpr (WARP) {
            const float* f = warp + i * 3;
            return warped_sample<DT, PT>(depth, p, e, i, f[0], f[1], f[2], a.rejected);
        } else {
            return depth_sample<DT, PT>(depth, p, e, i);
        }
    }
    __device__ bool fuse(const TsdfSample& s, long long i, float& t, float& W, const FusionDev& p, Acc& a) const {
        if (!fuse_voxel_weighted(s, pixel_weight, carve != 0, t, W, p, a.c.w)) return false;
        if (COLOUR == ALWAYS || (COLOUR == IF_GIVEN && c.volume != nullptr)) colour_voxel(s, pixel_weight, c, i, p, a.c);
        return true;
    }
    __device__ static void parts(const Acc& a, double (&v)[N]) {
        const WeightedAcc& w = a.c.w;
        v[0] = (double)w.a.fused; v[1] = (double)w.a.first; v[2] = w.a.sum; v[3] = (double)w.a.max;
        v[4] = (double)w.carved; v[5] = (double)w.rejected;
        if constexpr (N >= kCParts) { v[6] = (double)a.c.coloured; v[7] = (double)a.c.first; }
        if constexpr (N >= kXParts) v[8] = (double)a.rejected;
    }
};

// the walk
template <typename RULE>
__global__ __launch_bounds__(kBlock) void fusion_kernel(float* __restrict__ tsdf, float* __restrict__ weight, RULE rule,
                                                        double* __restrict__ scratch, FusionDev p) {
    constexpr int N = RULE::N;
    __shared__ double e[12];
    __shared__ double red[kBlock / kWave][N];
    if constexpr (RULE::kExtrinsic) {
        if (threadIdx.x == 0) live_extrinsic(p.twist, e);
        __syncthreads();
    }
    const bool aligned = p.aligned != 0;
    typename RULE::Acc a = {};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < p.groups; g += stride) {
        const long long i = g * 4;
        typename RULE::Obs o[4];
        float t[4], W[4];
        rule.observe4(i, p, e, o, a);
        load4(tsdf, i, t, aligned);
        load4(weight, i, W, aligned);
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) any = rule.fuse(o[k], i + k, t[k], W[k], p, a) || any;
        if (any) {  // a step without an updated voxel stores nothing; the stored values would equal the loaded ones
            store4(tsdf, i, t, aligned);
            store4(weight, i, W, aligned);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the tail, after this lane's steps
        for (long long i = p.groups * 4; i < p.n; ++i) {
            const typename RULE::Obs o = rule.observe(i, p, e, a);
            float t = tsdf[i], W = weight[i];
            if (rule.fuse(o, i, t, W, p, a)) {
                tsdf[i] = t;
                weight[i] = W;
            }
        }
    double v[N];
    RULE::parts(a, v);
    block_combine(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) scratch[(size_t)blockIdx.x * N + c] = v[c];
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

// the walk under a rule, then the combination of its partials into the record
template <typename RULE>
int launch(float* tsdf, float* weight, const RULE& rule, double* record, double* scratch, const FusionDev& p,
           hipStream_t s) {
    hipLaunchKernelGGL(fusion_kernel<RULE>, dim3(p.nblocks), dim3(kBlock), 0, s, tsdf, weight, rule, scratch, p);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(fusion_finish_kernel<RULE::N>, dim3(1), dim3(kBlock), 0, s, (const double*)scratch, record,
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

struct Buffer {
    const void* at;  // may be NULL: overlaps nothing
    size_t bytes;
};

// whether any two of the buffers share a byte
bool any_overlap(std::initializer_list<Buffer> buffers) {
    for (const Buffer* a = buffers.begin(); a != buffers.end(); ++a)
        for (const Buffer* b = a + 1; b != buffers.end(); ++b)
            if (overlaps(a->at, a->bytes, b->at, b->bytes)) return true;
    return false;
}

// a depth-mode call after the checks its four entry points share
struct DepthCall {
    FusionDev p;
    const lsf_fusion_params* f;
    double* scratch;
    hipStream_t s;
    size_t model, pixels, depth_bytes;  // the bytes of tsdf (and of weight), the image's pixels, the depth image's bytes
    int carve;
};

// those checks.  wp: the weighted parameters around f, NULL for the unweighted rule
int depth_call(const float* tsdf, const float* weight, const void* depth_image, const float* pixel_weight,
               const double* record, void* scratch, const lsf_fusion_params* f, const lsf_fusion_weighted_params* wp,
               void* stream, DepthCall& d) {
    if (int e = check_buffers(tsdf, weight, depth_image, record, scratch)) return e;
    if (int e = convert(f, d.p)) return e;
    if (!depth_dtype_ok(f->depth_dtype) || !typed_tsdf_ok(f->tsdf, false, true)) return LSF_ERR_BAD_ARGUMENT;
    if (wp && (wp->has_pixel_weight != 0) != (pixel_weight != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    d.p.aligned = aligned16(tsdf) && aligned16(weight);
    d.f = f;
    d.scratch = reinterpret_cast<double*>(scratch);
    d.s = as_stream(stream);
    d.model = (size_t)d.p.n * 4;
    d.pixels = (size_t)f->tsdf.image_width * f->tsdf.image_height;
    d.depth_bytes = d.pixels * kDepthBytes[f->depth_dtype];
    d.carve = wp && wp->carve != 0;
    return 0;
}

// make(DT(), PT()) gives the rule of the call's (depth dtype, intrinsics dtype); launched
template <typename MAKE>
int dispatch_rule(float* tsdf, float* weight, double* record, const DepthCall& d, MAKE&& make) {
    return dispatch_typed(d.f->depth_dtype, d.f->tsdf.intrinsics_are_f32 != 0, [&](auto dt, auto pt) {
        return launch(tsdf, weight, make(dt, pt), record, d.scratch, d.p, d.s);
    });
}

// the weighted rule with its buffers
template <bool WARP, int COLOUR, int PARTS>
int dispatch_weighted(float* tsdf, float* weight, const void* depth_image, const float* pixel_weight, const float* warp,
                    const ColourDev& c, double* record, const DepthCall& d) {
    return dispatch_rule(tsdf, weight, record, d, [&](auto dt, auto pt) {
        using DT = decltype(dt);
        return WeightedRule<DT, decltype(pt), WARP, COLOUR, PARTS>{reinterpret_cast<const DT*>(depth_image),
                                                                   pixel_weight, warp, c, d.carve, aligned16(warp)};
    });
}

}  // namespace

extern "C" int lsf_fusion_integrate_volume(float* tsdf, float* weight, const float* live, double* record,
                                           void* scratch, const lsf_fusion_params* params, void* stream) {
    (void)hipGetLastError();
    if (int e = check_buffers(tsdf, weight, live, record, scratch)) return e;
    FusionDev p;
    if (int e = convert(params, p)) return e;
    p.aligned = aligned16(tsdf) && aligned16(weight) && aligned16(live);
    return launch(tsdf, weight, VolumeRule{{}, live}, record, reinterpret_cast<double*>(scratch), p,
                  as_stream(stream));
}

extern "C" int lsf_fusion_integrate_depth(float* tsdf, float* weight, const void* depth_image, double* record,
                                          void* scratch, const lsf_fusion_params* params, void* stream) {
    (void)hipGetLastError();
    DepthCall d;
    if (int e = depth_call(tsdf, weight, depth_image, nullptr, record, scratch, params, nullptr, stream, d)) return e;
    return dispatch_rule(tsdf, weight, record, d, [&](auto dt, auto pt) {
        using DT = decltype(dt);
        return DepthRule<DT, decltype(pt)>{{}, reinterpret_cast<const DT*>(depth_image)};
    });
}

extern "C" int lsf_fusion_integrate_depth_weighted(float* tsdf, float* weight, const void* depth_image,
                                                   const float* pixel_weight, double* record, void* scratch,
                                                   const lsf_fusion_weighted_params* params, void* stream) {
    (void)hipGetLastError();
    if (!params) return LSF_ERR_BAD_ARGUMENT;
    DepthCall d;
    if (int e = depth_call(tsdf, weight, depth_image, pixel_weight, record, scratch, &params->fusion, params, stream, d))
        return e;
    if (overlaps(pixel_weight, d.pixels * 4, tsdf, d.model) || overlaps(pixel_weight, d.pixels * 4, weight, d.model))
        return LSF_ERR_BAD_ARGUMENT;
    return dispatch_weighted<false, NEVER, kWParts>(tsdf, weight, depth_image, pixel_weight, nullptr, ColourDev{}, record,
                                                  d);
}

extern "C" int lsf_fusion_integrate_depth_colour(float* tsdf, float* weight, float* colour, const void* depth_image,
                                                 const float* pixel_weight, const uint8_t* colour_image,
                                                 double* record, void* scratch, const lsf_fusion_colour_params* params,
                                                 void* stream) {
    (void)hipGetLastError();
    if (!params || !colour || !colour_image) return LSF_ERR_BAD_ARGUMENT;
    const lsf_fusion_weighted_params* wp = &params->weighted;
    DepthCall d;
    if (int e = depth_call(tsdf, weight, depth_image, pixel_weight, record, scratch, &wp->fusion, wp, stream, d))
        return e;
    const float band = params->colour_band;
    if (!(band > 0.0f && band <= 1.0f)) return LSF_ERR_BAD_ARGUMENT;  // NaN fails
    if (((uintptr_t)colour & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    if (any_overlap({{tsdf, d.model}, {weight, d.model}, {colour, d.model * 4}, {colour_image, d.pixels * 3},
                     {pixel_weight, d.pixels * 4}, {depth_image, d.depth_bytes}}))
        return LSF_ERR_BAD_ARGUMENT;
    const ColourDev c{reinterpret_cast<float4*>(colour), colour_image, band};
    return dispatch_weighted<false, ALWAYS, kCParts>(tsdf, weight, depth_image, pixel_weight, nullptr, c, record, d);
}

extern "C" int lsf_fusion_integrate_depth_warped(float* tsdf, float* weight, float* colour, const float* warp,
                                                 const void* depth_image, const float* pixel_weight,
                                                 const uint8_t* colour_image, double* record, void* scratch,
                                                 const lsf_fusion_warped_params* params, void* stream) {
    (void)hipGetLastError();
    if (!params || !warp) return LSF_ERR_BAD_ARGUMENT;
    const lsf_fusion_weighted_params* wp = &params->colour.weighted;
    DepthCall d;
    if (int e = depth_call(tsdf, weight, depth_image, pixel_weight, record, scratch, &wp->fusion, wp, stream, d))
        return e;
    const bool has_colour = params->has_colour != 0;
    if (has_colour != (colour != nullptr) || has_colour != (colour_image != nullptr)) return LSF_ERR_BAD_ARGUMENT;
    const float band = params->colour.colour_band;
    if (has_colour) {
        if (!(band > 0.0f && band <= 1.0f)) return LSF_ERR_BAD_ARGUMENT;  // NaN fails
        if (((uintptr_t)colour & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    }
    if (any_overlap({{tsdf, d.model}, {weight, d.model}, {colour, d.model * 4}, {warp, d.model * 3},
                     {depth_image, d.depth_bytes}, {pixel_weight, d.pixels * 4}, {colour_image, d.pixels * 3}}))
        return LSF_ERR_BAD_ARGUMENT;
    const ColourDev c{reinterpret_cast<float4*>(colour), colour_image, has_colour ? band : 1.0f};
    return dispatch_weighted<true, IF_GIVEN, kXParts>(tsdf, weight, depth_image, pixel_weight, warp, c, record, d);
}
