// The live depth pyramid (include/lsf_hip.h, lsf_depth_pyramid): KinectFusion's measurement stage in front of ICP,
// which the reference does not have.  The arithmetic is INTEGRATION.md section 3 ("Depth pyramid");
// tests/depth_pyramid_restatement.py restates it.  Every per-pixel step is one float64 operation in the order written
// there, and -ffp-contract=off keeps products and sums separately rounded.  levels + 1 launches, back to back:
//   filter     level 0: one lane per pixel, a workgroup per 16 x 16 tile; the tile and its radius-wide halo of scaled
//              depths are staged in LDS once, and the (2r + 1)^2 taps read them from there
//   downsample level l + 1 from level l: one lane per output pixel, the depth-gated mean of its 2 x 2 block
//   normals    every level in one launch: one lane per pixel of the whole pyramid, n = B x A of the forward differences
#include "lsf_device.h"
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kTile = 16;  // a filter workgroup covers 16 x 16 pixels
constexpr int kMaxLevels = LSF_ICP_MAX_LEVELS;
constexpr int kSide = kTile + 2 * LSF_PYRAMID_MAX_RADIUS;
static_assert(kTile * kTile == kBlock, "one lane per pixel of the tile");

struct FilterDev {
    double ratio, a, b;  // a = 1 / (2 sigma_space^2), b = 1 / (2 sigma_range^2)
    int height, width, radius;
};

struct NormalsDev {
    double fx[kMaxLevels], fy[kMaxLevels], cx[kMaxLevels], cy[kMaxLevels];
    long long offset[kMaxLevels + 1];  // level l's first pixel; offset[levels] = the pyramid's pixel count
    int height[kMaxLevels], width[kMaxLevels];
    int levels;
    double depth_gate;
};

template <typename DT>
__global__ __launch_bounds__(kBlock) void filter_kernel(const DT* __restrict__ depth, float* __restrict__ out,
                                                        FilterDev p) {
    __shared__ double tile[kSide * kSide];
    const int r = p.radius, side = kTile + 2 * r;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    // the tile and its halo; a cell outside the image holds 0, which no tap counts (0 is not valid)
    for (int c = threadIdx.x; c < side * side; c += kBlock) {
        const int gy = y0 - r + c / side, gx = x0 - r + c % side;
        tile[c] = (gx >= 0 && gx < p.width && gy >= 0 && gy < p.height)
                      ? (double)scaled_depth(depth, (long long)gy * p.width + gx, p.ratio)
                      : 0.0;
    }
    __syncthreads();
    const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= p.width || y >= p.height) return;
    const double* row = tile + (ly + r) * side + (lx + r);
    const double c = row[0];
    float value = 0.0f;
    if (c > 0.0) {  // NaN is not > 0
        if (r == 0) {
            value = (float)c;
        } else {
            double sw = 0.0, swd = 0.0;
            for (int dv = -r; dv <= r; ++dv)
                for (int du = -r; du <= r; ++du) {
                    const double d = row[dv * side + du];
                    if (d > 0.0) {
                        const double e = d - c;
                        const double w = exp(-((double)(du * du + dv * dv) * p.a + (e * e) * p.b));
                        sw += w;
                        swd += w * d;
                    }
                }
            value = (float)(swd / sw);
        }
    }
    out[(long long)y * p.width + x] = value;
}

// level l + 1 (extents h x w) from level l (row length w_in): the mean of the valid depths of the 2 x 2 block within
// depth_gate of its top-left one, 0 when that one is not valid
__global__ __launch_bounds__(kBlock) void downsample_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int h, int w, int w_in, double depth_gate) {
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= (long long)h * w) return;
    const int i = (int)(at / w), j = (int)(at % w);
    const float* q = in + (long long)(2 * i) * w_in + 2 * j;
    const double c = (double)q[0];
    float value = 0.0f;
    if (c > 0.0) {
        const double d[4] = {(double)q[0], (double)q[1], (double)q[w_in], (double)q[w_in + 1]};
        double sum = 0.0, count = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (d[k] > 0.0 && fabs(d[k] - c) <= depth_gate) {
                sum += d[k];
                count += 1.0;
            }
        value = (float)(sum / count);
    }
    out[at] = value;
}

__global__ __launch_bounds__(kBlock) void normals_kernel(const float* __restrict__ depth, float* __restrict__ normals,
                                                         NormalsDev p) {
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= p.offset[p.levels]) return;
    int l = 0;
    while (l + 1 < p.levels && at >= p.offset[l + 1]) ++l;
    const int w = p.width[l], h = p.height[l];
    const long long local = at - p.offset[l];
    const int v = (int)(local / w), u = (int)(local % w);
    double n[3] = {0.0, 0.0, 0.0};
    if (u + 1 < w && v + 1 < h) {
        const float* q = depth + at;
        const double d0 = (double)q[0], d1 = (double)q[1], d2 = (double)q[w];
        if (d0 > 0.0 && d1 > 0.0 && d2 > 0.0 && !(fabs(d1 - d0) > p.depth_gate) && !(fabs(d2 - d0) > p.depth_gate)) {
            const double fx = p.fx[l], fy = p.fy[l], cx = p.cx[l], cy = p.cy[l];
            const double xu = ((double)u - cx) / fx, xu1 = ((double)(u + 1) - cx) / fx;
            const double yv = ((double)v - cy) / fy, yv1 = ((double)(v + 1) - cy) / fy;
            const double V0[3] = {d0 * xu, d0 * yv, d0 * 1.0};
            const double V1[3] = {d1 * xu1, d1 * yv, d1 * 1.0};
            const double V2[3] = {d2 * xu, d2 * yv1, d2 * 1.0};
            double A[3], B[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { A[c] = V1[c] - V0[c]; B[c] = V2[c] - V0[c]; }
            const double m[3] = {B[1] * A[2] - B[2] * A[1], B[2] * A[0] - B[0] * A[2], B[0] * A[1] - B[1] * A[0]};
            const double norm = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            if (norm > 0.0)
#pragma unroll
                for (int c = 0; c < 3; ++c) n[c] = m[c] / norm;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[at * 3 + c] = (float)n[c];
}

unsigned blocks_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int lsf_depth_pyramid(const void* depth_image, float* pyramid_depth, float* pyramid_normals,
                                 const lsf_depth_pyramid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!depth_image || !pyramid_depth || !pyramid_normals || !params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_depth_pyramid_params* q = params;
    if (q->height < 1 || q->width < 1 || (long long)q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    for (double x : {q->fx, q->fy, q->cx, q->cy, q->depth_unit_ratio})
        if (!std::isfinite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->depth_gate > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (!depth_dtype_ok(q->depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    if (q->radius < 0 || q->radius > LSF_PYRAMID_MAX_RADIUS) return LSF_ERR_BAD_ARGUMENT;
    if (q->radius > 0)
        for (double s : {q->sigma_space, q->sigma_range})
            if (!(std::isfinite(s) && s > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (q->levels < 1 || q->levels > kMaxLevels || (q->height >> (q->levels - 1)) < 1 ||
        (q->width >> (q->levels - 1)) < 1)
        return LSF_ERR_BAD_ARGUMENT;
    NormalsDev nd;
    nd.levels = q->levels;
    nd.depth_gate = q->depth_gate;
    nd.offset[0] = 0;
    for (int l = 0; l < q->levels; ++l) {
        nd.height[l] = q->height >> l;
        nd.width[l] = q->width >> l;
        nd.offset[l + 1] = nd.offset[l] + (long long)nd.height[l] * nd.width[l];
        nd.fx[l] = l == 0 ? q->fx : nd.fx[l - 1] / 2.0;
        nd.fy[l] = l == 0 ? q->fy : nd.fy[l - 1] / 2.0;
        nd.cx[l] = l == 0 ? q->cx : (nd.cx[l - 1] - 0.5) / 2.0;
        nd.cy[l] = l == 0 ? q->cy : (nd.cy[l - 1] - 0.5) / 2.0;
    }
    static const size_t kDepthBytes[3] = {2, 4, 8};
    const size_t pixels = (size_t)nd.offset[q->levels];
    const size_t in_bytes = (size_t)q->height * q->width * kDepthBytes[q->depth_dtype];
    if (overlaps(depth_image, in_bytes, pyramid_depth, pixels * 4) ||
        overlaps(depth_image, in_bytes, pyramid_normals, pixels * 12) ||
        overlaps(pyramid_depth, pixels * 4, pyramid_normals, pixels * 12))
        return LSF_ERR_BAD_ARGUMENT;
    FilterDev fd;
    fd.ratio = q->depth_unit_ratio;
    fd.a = q->radius > 0 ? 1.0 / (2.0 * (q->sigma_space * q->sigma_space)) : 0.0;
    fd.b = q->radius > 0 ? 1.0 / (2.0 * (q->sigma_range * q->sigma_range)) : 0.0;
    fd.height = q->height;
    fd.width = q->width;
    fd.radius = q->radius;
    hipStream_t s = as_stream(stream);
    const dim3 tiles((q->width + kTile - 1) / kTile, (q->height + kTile - 1) / kTile);
    int e = dispatch_depth(q->depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        hipLaunchKernelGGL(filter_kernel<DT>, tiles, dim3(kBlock), 0, s, reinterpret_cast<const DT*>(depth_image),
                           pyramid_depth, fd);
        return launch_status();
    });
    for (int l = 1; l < q->levels && e == 0; ++l) {
        const long long n = (long long)nd.height[l] * nd.width[l];
        hipLaunchKernelGGL(downsample_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s, pyramid_depth + nd.offset[l - 1],
                           pyramid_depth + nd.offset[l], nd.height[l], nd.width[l], nd.width[l - 1], q->depth_gate);
        e = launch_status();
    }
    if (e) return e;
    hipLaunchKernelGGL(normals_kernel, dim3(blocks_of(nd.offset[q->levels])), dim3(kBlock), 0, s, pyramid_depth,
                       pyramid_normals, nd);
    return launch_status();
}
