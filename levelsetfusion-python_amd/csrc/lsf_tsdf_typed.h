// Nearest-pixel TSDF value of one voxel on the typed inputs of lsf_tsdf_generate_nearest_typed (reference
// tsdf/generation.py:130-207, :356-437; tsdf/common.py:34-47): uint16 / float32 / float64 depth, fractional array
// offsets, and an extrinsic evaluated in its own dtype.  Shared by lsf_tsdf.hip, the live-field stages of lsf_rigid.hip
// and lsf_rigid3d.hip, and depth-mode fusion (lsf_fusion.hip; the weighted rule also reads the pixel a voxel projects
// to, typed_tsdf_sample, and warped fusion samples at a displaced point, typed_tsdf_sample_at), as is the host-side
// setup at the end of this file (lsf_tsdf_params -> TypedTsdf, the depth-dtype and image checks, the (depth dtype,
// intrinsics dtype) dispatch).
// The dtypes are those numpy >= 2 gives the reference's expressions (oracle: tests/rigid_restatement.py):
//   voxel point     ((index + offset) * voxel_size) in float64, rounded to float32 (np.array(..., dtype=float32))
//   camera point    extrinsic.dot(point): float32 or float64 as the extrinsic, ((e0 x + e1 y) + e2 z) + e3
//   projection      promote(intrinsic dtype, camera point dtype); int() truncates
//   depth           uint16 * ratio and float64 * ratio in float64; float32 * ratio in float32 (a Python float is weak)
//   signed distance promote(depth dtype, camera point dtype); a float32 one meets float32(half width)
#pragma once

#include "lsf_device.h"

namespace lsf {

struct TypedTsdf {
    double fx, fy, cx, cy;
    double depth_unit_ratio, voxel_size, half_width;
    double off[3];
    int width, height, image_y;
    float default_value;
};

__device__ inline double scaled_depth(const unsigned short* d, long long i, double ratio) { return (double)d[i] * ratio; }
__device__ inline float scaled_depth(const float* d, long long i, double ratio) { return d[i] * (float)ratio; }
__device__ inline double scaled_depth(const double* d, long long i, double ratio) { return d[i] * ratio; }

template <typename S>
__device__ inline float typed_tsdf_value(S sd, double half) {
    const S h = (S)half;
    return sd < -h ? -1.0f : (sd > h ? 1.0f : (float)(sd / h));
}

template <typename Q>
__device__ inline long long typed_project(Q f, Q pc, Q z, Q c) {
    const Q v = ((f * pc) / z + c) + (Q)0.5;
    // int() of the reference truncates toward zero; saturate so that wild values stay out of range
    if (!(v > (Q)-2147483000.0 && v < (Q)2147483000.0)) return -1;
    return (long long)v;
}

// what a voxel sees of the depth image: its live value, and the pixel it projects to.  valid: the voxel lies in front of
// the camera, projects into the image and its pixel's scaled depth is > 0 or NaN (value is then not default_value, and
// pixel = iy * width + ix); otherwise value is default_value and pixel is -1.
struct TsdfSample {
    float value;
    long long pixel;
    bool valid;
};

// what the float32 point (xv, yv, zv), in the generator's metres, sees: everything of typed_tsdf_sample after the voxel
// point.  Warped depth fusion (lsf_fusion.hip) calls it with a voxel's point displaced by a warp field.
template <int D, typename E, typename P, typename DT>
__device__ inline TsdfSample typed_tsdf_sample_at(const DT* __restrict__ depth, const TypedTsdf& p, const E* e,
                                                  float xv, float yv, float zv) {
    using Q = decltype(E() + P());
    const TsdfSample none = {p.default_value, -1, false};
    const E pcx = ((e[0] * (E)xv + e[1] * (E)yv) + e[2] * (E)zv) + e[3] * (E)1;
    const E pcy = ((e[4] * (E)xv + e[5] * (E)yv) + e[6] * (E)zv) + e[7] * (E)1;
    const E pcz = ((e[8] * (E)xv + e[9] * (E)yv) + e[10] * (E)zv) + e[11] * (E)1;
    if (!(pcz > (E)0)) return none;
    const long long ix = typed_project<Q>((Q)(P)p.fx, (Q)pcx, (Q)pcz, (Q)(P)p.cx);
    const long long iy = D == 3 ? typed_project<Q>((Q)(P)p.fy, (Q)pcy, (Q)pcz, (Q)(P)p.cy) : (long long)p.image_y;
    if (ix < 0 || ix >= p.width || iy < 0 || iy >= p.height) return none;
    const long long pixel = iy * p.width + ix;
    const auto d = scaled_depth(depth, pixel, p.depth_unit_ratio);
    if (d <= 0) return none;  // NaN goes on, as in the reference
    using S = decltype(d + pcz);
    return {typed_tsdf_value<S>((S)d - (S)pcz, p.half_width), pixel, true};
}

// D = 2: field[y][x], x from the x index, the depth axis from the y index, y_voxel = 0, depth row p.image_y.
// D = 3: field[z][y][x].  E = float or double: the extrinsic's dtype (e: first three rows, row-major); P = the
// intrinsic matrix's dtype; DT = the depth image's element type.
template <int D, typename E, typename P, typename DT>
__device__ inline TsdfSample typed_tsdf_sample(const DT* __restrict__ depth, const TypedTsdf& p, const E* e, int x,
                                               int y, int z) {
    const float xv = (float)(((double)x + p.off[0]) * p.voxel_size);
    const float yv = D == 3 ? (float)(((double)y + p.off[1]) * p.voxel_size) : 0.0f;
    const float zv = (float)(((double)(D == 3 ? z : y) + p.off[2]) * p.voxel_size);
    return typed_tsdf_sample_at<D, E, P, DT>(depth, p, e, xv, yv, zv);
}

// the live value alone: what the generator, the trackers and unweighted fusion read
template <int D, typename E, typename P, typename DT>
__device__ inline float typed_tsdf_voxel(const DT* __restrict__ depth, const TypedTsdf& p, const E* e, int x, int y,
                                         int z) {
    return typed_tsdf_sample<D, E, P, DT>(depth, p, e, x, y, z).value;
}

// cv2.Rodrigues of a float64 rotation vector (math_utils/transformation.py::rodrigues), row-major
__device__ inline void rodrigues(const double r[3], double rot[9]) {
    const double theta = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    for (int i = 0; i < 9; ++i) rot[i] = i % 4 == 0 ? 1.0 : 0.0;
    if (theta < 2.220446049250313e-16) return;
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
    const double u[3] = {r[0] * itheta, r[1] * itheta, r[2] * itheta};
    const double rx[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            rot[i * 3 + j] = (c * (i == j ? 1.0 : 0.0) + c1 * (u[i] * u[j])) + s * rx[i * 3 + j];
}

// the live volume's extrinsic under a 6-DoF twist, rows 0..2 row-major: twist_vector_to_matrix3d of the float32-rounded
// twist (Rodrigues in float64 rounded to float32, as cv2.Rodrigues on a float32 vector), held in float64.  The rigid 3-D
// tracker (lsf_rigid3d.hip) and depth-mode fusion (lsf_fusion.hip) generate their live volumes under it.
__device__ inline void live_extrinsic(const double* tw, double* e) {
    double r[3], rot[9];
    for (int i = 0; i < 3; ++i) r[i] = (double)(float)tw[3 + i];
    rodrigues(r, rot);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) e[i * 4 + j] = (double)(float)rot[i * 3 + j];
        e[i * 4 + 3] = (double)(float)tw[i];
    }
}

// ---- host: the typed-TSDF setup of every entry point that generates from depth ------------------------------------

inline bool depth_dtype_ok(int32_t dt) { return dt == LSF_DEPTH_U16 || dt == LSF_DEPTH_F32 || dt == LSF_DEPTH_F64; }

// a depth element's bytes, by its checked LSF_DEPTH_* code
constexpr size_t kDepthBytes[3] = {2, 4, 8};

// the image and band checks of a typed-TSDF entry point.  image_y: the depth row must lie in the image (2-D);
// pixels: width x height must fit an int32.  Each entry point keeps the set of checks it has always made.
inline bool typed_tsdf_ok(const lsf_tsdf_params& t, bool image_y, bool pixels) {
    if (!(t.image_width > 0 && t.image_height > 0 && t.narrow_band_half_width > 0.0)) return false;
    if (image_y && (t.image_y_coordinate < 0 || t.image_y_coordinate >= t.image_height)) return false;
    return !pixels || (long long)t.image_width * t.image_height <= 0x7fffffffll;
}

inline TypedTsdf typed_tsdf(const lsf_tsdf_params& t, const double off[3], int image_y) {
    TypedTsdf p;
    p.fx = t.intrinsics[0]; p.fy = t.intrinsics[1]; p.cx = t.intrinsics[2]; p.cy = t.intrinsics[3];
    p.depth_unit_ratio = t.depth_unit_ratio;
    p.voxel_size = t.voxel_size;
    p.half_width = t.narrow_band_half_width;
    for (int i = 0; i < 3; ++i) p.off[i] = off[i];
    p.width = t.image_width; p.height = t.image_height; p.image_y = image_y;
    p.default_value = t.default_value;
    return p;
}

// f(DT()) with DT the element type of a checked LSF_DEPTH_* code; the argument carries its type only (decltype)
template <typename F>
inline int dispatch_depth(int32_t depth_dtype, F&& f) {
    if (depth_dtype == LSF_DEPTH_U16) return f((unsigned short)0);
    if (depth_dtype == LSF_DEPTH_F32) return f(float());
    return f(double());
}

// f(DT(), PT()), PT the intrinsics' type: one instantiation per (depth dtype, intrinsics dtype)
template <typename F>
inline int dispatch_typed(int32_t depth_dtype, bool intrinsics_f32, F&& f) {
    return dispatch_depth(depth_dtype, [&](auto dt) { return intrinsics_f32 ? f(dt, float()) : f(dt, double()); });
}

}  // namespace lsf
