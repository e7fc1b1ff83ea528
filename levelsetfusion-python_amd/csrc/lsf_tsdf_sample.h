// The weight-gated trilinear sample of the canonical TSDF, shared by the ray-caster (lsf_raycast.hip) and the
// point-to-SDF tracker (lsf_point_sdf.hip).  Internal linkage, as sample() had inside lsf_raycast.hip before it moved:
// the ray-cast kernels compile to the code they compiled to there (profiles/point_sdf_cost.md).
#pragma once

#include "lsf_device.h"

namespace {

struct Volume {
    const float* __restrict__ tsdf;
    const float* __restrict__ weight;
    int nx, ny, nz;
};

// the trilinear sample at voxel coordinates g; false when g is outside [0, n - 1) on an axis or a corner weight is
// not > 0
__device__ inline bool sample(const Volume& vol, double gx, double gy, double gz, double& value) {
    if (!(gx >= 0.0 && gx < (double)(vol.nx - 1) && gy >= 0.0 && gy < (double)(vol.ny - 1) && gz >= 0.0 &&
          gz < (double)(vol.nz - 1)))
        return false;
    const int x0 = (int)floor(gx), y0 = (int)floor(gy), z0 = (int)floor(gz);
    const long long sx = 1, sy = vol.nx, sz = (long long)vol.nx * vol.ny;
    const long long i = (long long)z0 * sz + (long long)y0 * sy + x0;
    const long long c[8] = {i, i + sx, i + sy, i + sy + sx, i + sz, i + sz + sx, i + sz + sy, i + sz + sy + sx};
    float w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = vol.weight[c[q]];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && w[q] > 0.0f;  // NaN is not > 0
    if (!ok) return false;
    float t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = vol.tsdf[c[q]];
    const double fx = gx - (double)x0, fy = gy - (double)y0, fz = gz - (double)z0;
    const double hx = 1.0 - fx, hy = 1.0 - fy, hz = 1.0 - fz;
    const double c00 = (double)t[0] * hx + (double)t[1] * fx;  // z0 y0
    const double c01 = (double)t[2] * hx + (double)t[3] * fx;  // z0 y1
    const double c10 = (double)t[4] * hx + (double)t[5] * fx;  // z1 y0
    const double c11 = (double)t[6] * hx + (double)t[7] * fx;  // z1 y1
    const double c0 = c00 * hy + c01 * fy;
    const double c1 = c10 * hy + c11 * fy;
    value = c0 * hz + c1 * fz;
    return true;
}

// the trilinear interpolant of the 8 corner values t0 .. t7 (x fastest, then y, then z) at the fractions f, h = 1 - f,
// and its gradient in voxel units, d = (d/dx, d/dy, d/dz) ("Point-to-SDF tracking")
__device__ inline void trilinear_gradient(const double (&t)[8], const double (&f)[3], const double (&h)[3],
                                          double& value, double (&d)[3]) {
    const double fx = f[0], fy = f[1], fz = f[2], hx = h[0], hy = h[1], hz = h[2];
    const double c00 = t[0] * hx + t[1] * fx;  // z0 y0
    const double c01 = t[2] * hx + t[3] * fx;  // z0 y1
    const double c10 = t[4] * hx + t[5] * fx;  // z1 y0
    const double c11 = t[6] * hx + t[7] * fx;  // z1 y1
    const double c0 = c00 * hy + c01 * fy;
    const double c1 = c10 * hy + c11 * fy;
    value = c0 * hz + c1 * fz;
    d[0] = ((t[1] - t[0]) * hy + (t[3] - t[2]) * fy) * hz + ((t[5] - t[4]) * hy + (t[7] - t[6]) * fy) * fz;
    d[1] = (c01 - c00) * hz + (c11 - c10) * fz;
    d[2] = c1 - c0;
}

// the cell of a sample: its lowest corner's index in the volume and the fractions f on x, y, z
struct Cell {
    long long at;
    double f[3];
};

// the indices of a cell's 8 corners, x fastest, then y, then z
__device__ inline void cell_corners(const Volume& vol, long long i, long long (&c)[8]) {
    const long long sx = 1, sy = vol.nx, sz = (long long)vol.nx * vol.ny;
    c[0] = i; c[1] = i + sx; c[2] = i + sy; c[3] = i + sy + sx;
    c[4] = i + sz; c[5] = i + sz + sx; c[6] = i + sz + sy; c[7] = i + sz + sy + sx;
}

// sample() and the gradient of its interpolant in voxel units from the same 8 corners: value and validity are
// sample()'s bit for bit; cell: where the sample was taken
__device__ inline bool sample_gradient(const Volume& vol, double gx, double gy, double gz, double& value,
                                       double (&d)[3], Cell& cell) {
    if (!(gx >= 0.0 && gx < (double)(vol.nx - 1) && gy >= 0.0 && gy < (double)(vol.ny - 1) && gz >= 0.0 &&
          gz < (double)(vol.nz - 1)))
        return false;
    const int x0 = (int)floor(gx), y0 = (int)floor(gy), z0 = (int)floor(gz);
    cell.at = (long long)z0 * ((long long)vol.nx * vol.ny) + (long long)y0 * vol.nx + x0;
    long long c[8];
    cell_corners(vol, cell.at, c);
    float w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = vol.weight[c[q]];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) ok = ok && w[q] > 0.0f;  // NaN is not > 0
    if (!ok) return false;
    double t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = (double)vol.tsdf[c[q]];
    cell.f[0] = gx - (double)x0; cell.f[1] = gy - (double)y0; cell.f[2] = gz - (double)z0;
    const double h[3] = {1.0 - cell.f[0], 1.0 - cell.f[1], 1.0 - cell.f[2]};
    trilinear_gradient(t, cell.f, h, value, d);
    return true;
}

}  // namespace
