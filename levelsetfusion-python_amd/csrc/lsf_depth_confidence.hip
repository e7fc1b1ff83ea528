// The per-pixel confidence image of weighted fusion (include/lsf_hip.h, lsf_depth_confidence), which the reference does
// not have.  The arithmetic is INTEGRATION.md section 3 ("Depth confidence"); tests/fusion_weighted_restatement.py
// restates it.  For pixel (u, v) with depth z (metres) and camera-space normal n, every step one float64 operation in
// this order, and -ffp-contract=off keeps products and sums separately rounded:
//   x = (u - cx) / fx,  y = (v - cy) / fy,  len = sqrt((x x + y y) + 1)      the ray (x, y, 1) and its length
//   dot = (n_x x + n_y y) + n_z,  a = |dot| / len                            |n . r|, r the unit ray
//   q = z_ref / z,  s = q q,  m = s < 1 ? s : 1                              min(1, (z_ref / z)^2)
//   c = (float)(a m)                                                         rounded once
// c = 0 where z is not > 0 (a hole or NaN) and where the normal is the depth pyramid's "no normal" value: the zero
// vector, which lsf_depth_pyramid.hip's normals kernel writes at the last row and column, at invalid depths, across a
// depth step wider than its gate and where the cross product vanishes.
// One lane per pixel; a workgroup covers a 64 x 4 tile, so a wave reads 256 contiguous bytes of depth.  One launch.
#include "lsf_device.h"

using namespace lsf;

namespace {

struct ConfidenceDev {
    double fx, fy, cx, cy, z_ref;
    int height, width;
};

__global__ __launch_bounds__(kBlock) void confidence_kernel(const float* __restrict__ depth,
                                                            const float* __restrict__ normals,
                                                            float* __restrict__ out, ConfidenceDev p) {
    const int u = blockIdx.x * kTileX + threadIdx.x % kTileX, v = blockIdx.y * kTileY + threadIdx.x / kTileX;
    if (u >= p.width || v >= p.height) return;
    const long long at = (long long)v * p.width + u;
    const double z = (double)depth[at];
    const double nx = (double)normals[at * 3], ny = (double)normals[at * 3 + 1], nz = (double)normals[at * 3 + 2];
    float c = 0.0f;
    if (z > 0.0 && !(nx == 0.0 && ny == 0.0 && nz == 0.0)) {  // NaN is not > 0
        const double x = ((double)u - p.cx) / p.fx, y = ((double)v - p.cy) / p.fy;
        const double len = sqrt((x * x + y * y) + 1.0);
        const double dot = (nx * x + ny * y) + nz;
        const double a = fabs(dot) / len;
        const double q = p.z_ref / z;
        const double s = q * q;
        const double m = s < 1.0 ? s : 1.0;
        c = (float)(a * m);
    }
    out[at] = c;
}

}  // namespace

extern "C" int lsf_depth_confidence(const float* depth, const float* normals, float* confidence_out,
                                    const lsf_depth_confidence_params* params, void* stream) {
    (void)hipGetLastError();
    if (!depth || !normals || !confidence_out || !params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_depth_confidence_params* q = params;
    if (q->height < 1 || q->width < 1 || (long long)q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    for (double x : {q->fx, q->fy, q->cx, q->cy, q->reference_depth})
        if (!std::isfinite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (q->fx == 0.0 || q->fy == 0.0 || !(q->reference_depth > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    const size_t pixels = (size_t)q->height * q->width;
    if (overlaps(confidence_out, pixels * 4, depth, pixels * 4) ||
        overlaps(confidence_out, pixels * 4, normals, pixels * 12))
        return LSF_ERR_BAD_ARGUMENT;
    const ConfidenceDev p = {q->fx, q->fy, q->cx, q->cy, q->reference_depth, q->height, q->width};
    const dim3 tiles((q->width + kTileX - 1) / kTileX, (q->height + kTileY - 1) / kTileY);
    if (tiles.y > 65535u) return LSF_ERR_BAD_ARGUMENT;  // the grid's y extent
    hipLaunchKernelGGL(confidence_kernel, tiles, dim3(kBlock), 0, as_stream(stream), depth, normals, confidence_out, p);
    return launch_status();
}
