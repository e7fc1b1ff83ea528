// Ray-casting the canonical TSDF into a depth and normal image (include/lsf_hip.h, lsf_raycast): the model rendering
// of KillingFusion-style tracking, which the reference does not have.  The arithmetic is INTEGRATION.md section 3
// ("Ray-casting"); tests/raycast_restatement.py restates it and the kernel equals it bit for bit.  Every step is one
// float64 operation in the order written there; -ffp-contract=off keeps products and sums separately rounded.
// One lane per pixel.  A workgroup of 4 waves covers a 16 x 16 pixel tile, each wave an 8 x 8 block, so that the 64
// rays of a wave stay within a few voxels of each other and their trilinear gathers share cache lines.  The march is a
// fixed step of voxel_size / 2 in camera z on a grid of sample positions shared by all rays (s = m * step), clipped to
// the volume's box with a one-step pad: the clip decides only where a lane starts and stops, never what a sample is.
// The 8 corner weights of a sample are read first; its 8 tsdf values only when all weights are > 0.
// lsf_raycast_colour is the same kernel with COLOUR set: after the march a hit pixel also samples the model's colour
// records at its hit point ("Ray-cast colour"), the 8 colour weights first.
#include "lsf_device.h"
#include "lsf_tsdf_sample.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kTile = LSF_RAYCAST_TILE;
constexpr int kSub = 8;  // a wave's pixel block is kSub x kSub
static_assert(kSub * kSub == kWave && (kTile / kSub) * (kTile / kSub) * kWave == kBlock, "4 waves of 8 x 8 pixels");

struct RayDev {
    double fx, fy, cx, cy, ratio, voxel, step;
    double off[3];
    double twist[6];
    int n[3];               // extents x, y, z
    int height, width;
    long long max_steps;    // a defensive bound on a ray's steps, above what any ray through the box takes
};

// the trilinear sample of R, G, B (records of 4 floats, the colour weight last) at voxel coordinates g, in sample()'s
// order per channel; false when a corner lies outside the volume or a colour weight is not > 0
__device__ inline bool sample_colour(const Volume& vol, const float* __restrict__ colour, double gx, double gy,
                                     double gz, double (&rgb)[3]) {
    if (!(gx >= 0.0 && gx < (double)(vol.nx - 1) && gy >= 0.0 && gy < (double)(vol.ny - 1) && gz >= 0.0 &&
          gz < (double)(vol.nz - 1)))
        return false;
    const int x0 = (int)floor(gx), y0 = (int)floor(gy), z0 = (int)floor(gz);
    const long long sx = 1, sy = vol.nx, sz = (long long)vol.nx * vol.ny;
    const long long i = (long long)z0 * sz + (long long)y0 * sy + x0;
    const long long c[8] = {i, i + sx, i + sy, i + sy + sx, i + sz, i + sz + sx, i + sz + sy, i + sz + sy + sx};
    float w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = colour[c[q] * 4 + 3];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && w[q] > 0.0f;  // NaN is not > 0
    if (!ok) return false;
    const double fx = gx - (double)x0, fy = gy - (double)y0, fz = gz - (double)z0;
    const double hx = 1.0 - fx, hy = 1.0 - fy, hz = 1.0 - fz;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = colour[c[q] * 4 + ch];
        const double c00 = (double)t[0] * hx + (double)t[1] * fx;
        const double c01 = (double)t[2] * hx + (double)t[3] * fx;
        const double c10 = (double)t[4] * hx + (double)t[5] * fx;
        const double c11 = (double)t[6] * hx + (double)t[7] * fx;
        const double c0 = c00 * hy + c01 * fy;
        const double c1 = c10 * hy + c11 * fy;
        rgb[ch] = c0 * hz + c1 * fz;
    }
    return true;
}

__device__ inline double dmin(double a, double b) { return b < a ? b : a; }
__device__ inline double dmax(double a, double b) { return b > a ? b : a; }

template <typename DT, bool COLOUR>
__global__ __launch_bounds__(kBlock) void raycast_kernel(Volume vol, const DT* __restrict__ fallback,
                                                         float* __restrict__ depth_out,
                                                         float* __restrict__ normals_out,
                                                         unsigned long long* __restrict__ hit_count, RayDev p,
                                                         const float* __restrict__ colour,
                                                         float* __restrict__ colour_out) {
    __shared__ double e_sh[12];
    if (threadIdx.x == 0) live_extrinsic(p.twist, e_sh);
    __syncthreads();
    double e[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) e[q] = e_sh[q];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int u = blockIdx.x * kTile + (wave % (kTile / kSub)) * kSub + lane % kSub;
    const int v = blockIdx.y * kTile + (wave / (kTile / kSub)) * kSub + lane / kSub;
    const bool inside = u < p.width && v < p.height;
    bool hit = false;
    double s_hit = 0.0;
    double a[3], b[3];
    if (inside) {
        const double dcx = ((double)u - p.cx) / p.fx, dcy = ((double)v - p.cy) / p.fy;
        // g(s) = a + s b: the ray in voxel coordinates, o = -R^T t, d = R^T (dcx, dcy, 1)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double o = -((e[j] * e[3] + e[4 + j] * e[7]) + e[8 + j] * e[11]);
            const double d = (e[j] * dcx + e[4 + j] * dcy) + e[8 + j] * 1.0;
            a[j] = o / p.voxel - p.off[j];
            b[j] = d / p.voxel;
        }
        double lo = -INFINITY, hi = INFINITY;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double top = (double)(p.n[j] - 1);
            if (b[j] != 0.0) {
                const double s1 = (0.0 - a[j]) / b[j], s2 = (top - a[j]) / b[j];
                lo = dmax(lo, dmin(s1, s2));
                hi = dmin(hi, dmax(s1, s2));
            } else if (!(a[j] >= 0.0 && a[j] < top)) {
                lo = INFINITY;
                hi = -INFINITY;
            }
        }
        if (lo <= hi && hi > 0.0 && hi / p.step < 1125899906842624.0) {  // 2^50
            const long long k0 = (long long)dmax(floor(lo / p.step) - 1.0, 1.0);
            long long k1 = (long long)(floor(hi / p.step) + 1.0);
            if (k1 > k0 + p.max_steps) k1 = k0 + p.max_steps;
            bool prev_valid = false;
            double prev = 0.0;
            for (long long m = k0; m <= k1; ++m) {
                const double s = (double)m * p.step;
                double val = 0.0;
                const bool valid = sample(vol, a[0] + s * b[0], a[1] + s * b[1], a[2] + s * b[2], val);
                if (prev_valid && prev > 0.0 && valid && val <= 0.0) {
                    s_hit = (double)(m - 1) * p.step + p.step * (prev / (prev - val));
                    hit = true;
                    break;
                }
                prev_valid = valid;
                prev = val;
            }
        }
    }
    if (hit_count) {
        const unsigned long long mask = __ballot(hit);
        if (lane == 0 && mask) atomicAdd(hit_count, (unsigned long long)__popcll(mask));
    }
    if (!inside) return;
    const long long px = (long long)v * p.width + u;
    float out = (float)s_hit;
    if (!hit) out = fallback ? (float)scaled_depth(fallback, px, p.ratio) : 0.0f;
    depth_out[px] = out;
    if constexpr (COLOUR) {  // (R, G, B, Y) at the unrounded hit point, four NaNs without a hit or a colour
        float rgby[4] = {NAN, NAN, NAN, NAN};
        double rgb[3];
        if (hit && sample_colour(vol, colour, a[0] + s_hit * b[0], a[1] + s_hit * b[1], a[2] + s_hit * b[2], rgb)) {
            const double y = ((0.299 * rgb[0] + 0.587 * rgb[1]) + 0.114 * rgb[2]) / 255.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) rgby[i] = (float)rgb[i];
            rgby[3] = (float)y;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) colour_out[px * 4 + i] = rgby[i];
    }
    if (!normals_out) return;
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
        const double g[3] = {a[0] + s_hit * b[0], a[1] + s_hit * b[1], a[2] + s_hit * b[2]};
        double grad[3];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double gp[3] = {g[0], g[1], g[2]}, gm[3] = {g[0], g[1], g[2]};
            gp[j] = g[j] + 1.0;
            gm[j] = g[j] - 1.0;
            double vp = 0.0, vm = 0.0;
            const bool a_ok = sample(vol, gp[0], gp[1], gp[2], vp);
            const bool b_ok = sample(vol, gm[0], gm[1], gm[2], vm);
            ok = ok && a_ok && b_ok;
            grad[j] = vp - vm;
        }
        if (ok) {
            double nc[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) nc[i] = (e[i * 4] * grad[0] + e[i * 4 + 1] * grad[1]) + e[i * 4 + 2] * grad[2];
            const double len2 = (nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2];
            if (len2 > 0.0) {
                const double len = sqrt(len2);
#pragma unroll
                for (int i = 0; i < 3; ++i) nrm[i] = (float)(nc[i] / len);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) normals_out[px * 3 + i] = nrm[i];
}

bool finite(double x) { return std::isfinite(x); }

int convert(const lsf_raycast_params* q, bool with_fallback, RayDev& p) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->depth < 2 || q->height < 2 || q->width < 2) return LSF_ERR_BAD_ARGUMENT;
    if (q->image_height < 1 || q->image_width < 1 || (long long)q->image_height * q->image_width > 0x7fffffffll)
        return LSF_ERR_BAD_ARGUMENT;
    const double all[] = {q->fx, q->fy, q->cx, q->cy, q->voxel_size, q->offset_x, q->offset_y, q->offset_z,
                          q->t_x, q->t_y, q->t_z, q->r_x, q->r_y, q->r_z};
    for (double x : all)
        if (!finite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->voxel_size > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (with_fallback && (!depth_dtype_ok(q->fallback_dtype) || !finite(q->depth_unit_ratio)))
        return LSF_ERR_BAD_ARGUMENT;
    p.fx = q->fx; p.fy = q->fy; p.cx = q->cx; p.cy = q->cy;
    p.ratio = q->depth_unit_ratio;
    p.voxel = q->voxel_size;
    p.step = q->voxel_size / LSF_RAYCAST_STEPS_PER_VOXEL;
    p.off[0] = q->offset_x; p.off[1] = q->offset_y; p.off[2] = q->offset_z;
    const double tw[6] = {q->t_x, q->t_y, q->t_z, q->r_x, q->r_y, q->r_z};
    for (int i = 0; i < 6; ++i) p.twist[i] = tw[i];
    p.n[0] = q->width; p.n[1] = q->height; p.n[2] = q->depth;
    p.height = q->image_height;
    p.width = q->image_width;
    p.max_steps = 4ll * ((long long)q->width + q->height + q->depth) + 8;
    return 0;
}

template <typename DT, bool COLOUR>
int launch(const Volume& vol, const void* fallback, float* depth_out, float* normals_out, uint64_t* hits,
           const RayDev& p, const float* colour, float* colour_out, hipStream_t s) {
    const dim3 grid((unsigned)((p.width + kTile - 1) / kTile), (unsigned)((p.height + kTile - 1) / kTile));
    hipLaunchKernelGGL((raycast_kernel<DT, COLOUR>), grid, dim3(kBlock), 0, s, vol,
                       reinterpret_cast<const DT*>(fallback), depth_out, normals_out,
                       reinterpret_cast<unsigned long long*>(hits), p, colour, colour_out);
    return launch_status();
}

// both entry points: colour and colour_out are NULL from lsf_raycast
template <bool COLOUR>
int raycast(const float* tsdf, const float* weight, const float* colour, const void* fallback_depth, float* depth_out,
            float* normals_out, float* colour_out, uint64_t* hit_count, const lsf_raycast_params* params,
            void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || !depth_out || tsdf == weight) return LSF_ERR_BAD_ARGUMENT;
    if (COLOUR && (!colour || !colour_out)) return LSF_ERR_BAD_ARGUMENT;
    RayDev p;
    if (int e = convert(params, fallback_depth != nullptr, p)) return e;
    const size_t voxels = (size_t)params->depth * params->height * params->width * 4;
    const size_t pixels = (size_t)p.height * p.width;
    static const size_t kDepthBytes[3] = {2, 4, 8};
    const size_t fb = fallback_depth ? pixels * kDepthBytes[params->fallback_dtype] : 0;
    // no output may alias an input or another output
    const void* outs[4] = {depth_out, normals_out, hit_count, colour_out};
    const size_t out_bytes[4] = {pixels * 4, pixels * 12, 8, pixels * 16};
    const void* ins[4] = {tsdf, weight, fallback_depth, colour};
    const size_t in_bytes[4] = {voxels, voxels, fb, voxels * 4};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j)
            if (overlaps(outs[i], out_bytes[i], ins[j], in_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    }
    const Volume vol{tsdf, weight, params->width, params->height, params->depth};
    hipStream_t s = as_stream(stream);
    if (!fallback_depth)
        return launch<float, COLOUR>(vol, nullptr, depth_out, normals_out, hit_count, p, colour, colour_out, s);
    return dispatch_depth(params->fallback_dtype, [&](auto dt) {
        return launch<decltype(dt), COLOUR>(vol, fallback_depth, depth_out, normals_out, hit_count, p, colour,
                                            colour_out, s);
    });
}

}  // namespace

extern "C" int lsf_raycast(const float* tsdf, const float* weight, const void* fallback_depth, float* depth_out,
                           float* normals_out, uint64_t* hit_count, const lsf_raycast_params* params, void* stream) {
    return raycast<false>(tsdf, weight, nullptr, fallback_depth, depth_out, normals_out, nullptr, hit_count, params,
                          stream);
}

extern "C" int lsf_raycast_colour(const float* tsdf, const float* weight, const float* colour,
                                  const void* fallback_depth, float* depth_out, float* normals_out, float* colour_out,
                                  uint64_t* hit_count, const lsf_raycast_params* params, void* stream) {
    return raycast<true>(tsdf, weight, colour, fallback_depth, depth_out, normals_out, colour_out, hit_count, params,
                         stream);
}
