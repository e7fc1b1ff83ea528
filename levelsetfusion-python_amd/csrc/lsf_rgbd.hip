// The RGB-D sensor front end (include/lsf_hip.h, lsf_rgbd_ray_table / _register_depth / _rectify_colour; INTEGRATION.md
// section 3, "RGB-D sensor"; tests/rgbd_restatement.py restates it): the undistorted rays of a lens as a table, a raw depth
// image registered into an ideal pinhole camera through a z-buffer, and a raw colour image resampled into that camera.
// Every float step is float64 and written as the header writes it: the build's -ffp-contract=off keeps a multiply and an
// add apart, so the outputs are the numpy restatement's bit for bit.
// Shape.  One lane per pixel (of the source in the table and the splat, of the output in the clear, finalise and rectify
// launches), 256 lanes along rows: a lane's table reads are 16 bytes next to its neighbour's, the image accesses 2 to 8.
// A capped grid with a stride loop behind it.  The z-buffer takes HIP's unsigned atomicMin, at most max_footprint^2 per
// lane; positive finite floats order as their bits, so the minimum is the nearest surface whatever the order.  The
// record's counts are summed per wave by shuffles, per workgroup through four LDS words, and added with one integer atomic
// per workgroup and non-zero count, exact in any order.  (One atomic per WAVE was measured first: ~9000 adds on one cache
// line serialise at ~13 ns each and made a 640 x 480 call 117 us, the same at every size.)  `valid` takes no atomic at
// all: it is the sum of the four fates, which the finalise launch forms once the splat is complete.
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kMaxBlocks = LSF_RGBD_MAX_BLOCKS;
constexpr int kIterations = LSF_RGBD_UNDISTORT_ITERATIONS;
constexpr unsigned kEmpty = LSF_RGBD_ZBUFFER_EMPTY;
constexpr double kIntLimit = 2147483000.0;
enum { kValid, kBehind, kOutside, kEmptyRange, kClipped, kWritten, kFilled, kMasked };
static_assert(kMasked + 1 == LSF_RGBD_RECORD_WORDS, "the record's eight counts");

struct Lens {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
    int pinhole;  // all eight coefficients are 0: no iteration, the ray is exact
};

struct Pinhole {
    double fx, fy, cx, cy;
};

struct Rigid {
    double r[9], t[3];
};

// the tangential part and the two radial polynomials at (x, y)
struct Radial {
    double num, den, dx, dy;
};

__device__ inline Radial radial_at(const Lens& l, double x, double y) {
    Radial r;
    const double r2 = x * x + y * y;
    r.num = 1.0 + r2 * (l.k1 + r2 * (l.k2 + r2 * l.k3));
    r.den = 1.0 + r2 * (l.k4 + r2 * (l.k5 + r2 * l.k6));
    r.dx = 2.0 * l.p1 * x * y + l.p2 * (r2 + 2.0 * x * x);
    r.dy = l.p1 * (r2 + 2.0 * y * y) + 2.0 * l.p2 * x * y;
    return r;
}

__device__ inline void distort(const Lens& l, double x, double y, double& xd, double& yd) {
    const Radial r = radial_at(l, x, y);
    const double s = r.num / r.den;
    xd = x * s + r.dx;
    yd = y * s + r.dy;
}

// the normalised coordinates whose distorted image is pixel (pu, pv): kIterations fixed-point steps, no early exit
__device__ inline double2 undistorted_ray(const Lens& l, double pu, double pv) {
    const double xd = (pu - l.cx) / l.fx, yd = (pv - l.cy) / l.fy;
    double x = xd, y = yd;
    if (!l.pinhole) {
        for (int it = 0; it < kIterations; ++it) {
            const Radial r = radial_at(l, x, y);
            const double xn = (xd - r.dx) * r.den / r.num;
            const double yn = (yd - r.dy) * r.den / r.num;
            x = xn;
            y = yn;
        }
    }
    return make_double2(x, y);
}

// lane i of the (height + 1) x (width + 1) corner lattice writes its corner and, inside the image, the centre of pixel (u, v)
__global__ __launch_bounds__(kBlock) void rgbd_ray_table_kernel(double2* __restrict__ corner, double2* __restrict__ centre,
                                                                Lens l, int height, int width) {
    const int cw = width + 1;
    const long long total = (long long)(height + 1) * cw;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int v = (int)(i / cw), u = (int)(i - (long long)v * cw);
        corner[i] = undistorted_ray(l, (double)u - 0.5, (double)v - 0.5);
        if (u < width && v < height) centre[(long long)v * width + u] = undistorted_ray(l, (double)u, (double)v);
    }
}

__global__ __launch_bounds__(kBlock) void rgbd_clear_kernel(unsigned* __restrict__ zbuffer, long long* __restrict__ record,
                                                            long long pixels) {
    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (first < LSF_RGBD_RECORD_WORDS) record[first] = 0;
    for (long long i = first; i < pixels; i += stride) zbuffer[i] = kEmpty;
}

// the workgroup's sum of a lane count, added to *dst by one lane when it is not 0: shuffles inside a wave, one LDS word
// per wave across them.  Every thread of the workgroup must call it.
__device__ inline void block_count_commit(int mine, long long* dst) {
    __shared__ int s_wave[kBlock / kWave];
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) mine += __shfl_down(mine, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) all += s_wave[w];
        if (all != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)all);
    }
    __syncthreads();
}

__device__ inline void move_point(const Rigid& g, double p0, double p1, double p2, double (&q)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = ((g.r[i * 3] * p0 + g.r[i * 3 + 1] * p1) + g.r[i * 3 + 2] * p2) + g.t[i];
}

template <typename DT>
__global__ __launch_bounds__(kBlock) void rgbd_splat_kernel(const DT* __restrict__ depth,
                                                            const double2* __restrict__ corner,
                                                            const double2* __restrict__ centre,
                                                            unsigned* __restrict__ zbuffer, long long* __restrict__ record,
                                                            Rigid g, Pinhole o, double ratio, int height, int width,
                                                            int out_height, int out_width, int max_footprint) {
    const long long total = (long long)height * width;
    const long long stride = (long long)gridDim.x * kBlock;
    int n_behind = 0, n_outside = 0, n_empty = 0, n_clipped = 0, n_written = 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const double z = (double)scaled_depth(depth, i, ratio);
        if (!(z > 0.0 && z <= 1.7976931348623157e308)) continue;  // 0, negative, NaN, inf: no measurement
        const int v = (int)((unsigned)i / (unsigned)width), u = (int)(i - (long long)v * width);  // i < 2^31
        const double2 c = centre[i];
        double q[3];
        move_point(g, c.x * z, c.y * z, z, q);
        const float zf = (float)q[2];
        if (!(q[2] > 0.0) || !(zf <= 3.402823466e+38f)) {
            ++n_behind;
            continue;
        }
        const long long row0 = (long long)v * (width + 1) + u, row1 = row0 + (width + 1);
        const double2 ray[4] = {corner[row0], corner[row0 + 1], corner[row1], corner[row1 + 1]};
        double lo_u = 0.0, hi_u = 0.0, lo_v = 0.0, hi_v = 0.0;
        bool behind = false, finite = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double qc[3];
            move_point(g, ray[j].x * z, ray[j].y * z, z, qc);
            behind = behind || qc[2] <= 0.0;
            const double pu = o.fx * (qc[0] / qc[2]) + o.cx, pv = o.fy * (qc[1] / qc[2]) + o.cy;
            finite = finite && fabs(pu) <= 1.7976931348623157e308 && fabs(pv) <= 1.7976931348623157e308;  // false for NaN
            lo_u = j == 0 ? pu : fmin(lo_u, pu);
            hi_u = j == 0 ? pu : fmax(hi_u, pu);
            lo_v = j == 0 ? pv : fmin(lo_v, pv);
            hi_v = j == 0 ? pv : fmax(hi_v, pv);
        }
        if (behind) {
            ++n_behind;
            continue;
        }
        const double bu0 = ceil(lo_u), bu1 = ceil(hi_u), bv0 = ceil(lo_v), bv1 = ceil(hi_v);
        if (!finite || bu0 < -kIntLimit || bu1 > kIntLimit || bv0 < -kIntLimit || bv1 > kIntLimit) {
            ++n_outside;
            continue;
        }
        long long u0 = (long long)bu0, u1 = (long long)bu1, v0 = (long long)bv0, v1 = (long long)bv1;
        bool clipped = false;
        if (u1 - u0 > max_footprint) {
            u1 = u0 + max_footprint;
            clipped = true;
        }
        if (v1 - v0 > max_footprint) {
            v1 = v0 + max_footprint;
            clipped = true;
        }
        n_clipped += clipped ? 1 : 0;
        if (u0 >= u1 || v0 >= v1) {
            ++n_empty;
            continue;
        }
        if (u1 <= 0 || v1 <= 0 || u0 >= out_width || v0 >= out_height) {
            ++n_outside;
            continue;
        }
        ++n_written;
        const int a0 = (int)(u0 < 0 ? 0 : u0), a1 = (int)(u1 > out_width ? out_width : u1);
        const int b0 = (int)(v0 < 0 ? 0 : v0), b1 = (int)(v1 > out_height ? out_height : v1);
        const unsigned bits = __float_as_uint(zf);
        for (int y = b0; y < b1; ++y)
            for (int x = a0; x < a1; ++x) atomicMin(zbuffer + ((long long)y * out_width + x), bits);
    }
    block_count_commit(n_behind, record + kBehind);
    block_count_commit(n_outside, record + kOutside);
    block_count_commit(n_empty, record + kEmptyRange);
    block_count_commit(n_clipped, record + kClipped);
    block_count_commit(n_written, record + kWritten);
}

__global__ __launch_bounds__(kBlock) void rgbd_finalise_kernel(const unsigned* __restrict__ zbuffer,
                                                               const unsigned char* __restrict__ colour_valid,
                                                               float* __restrict__ out_depth,
                                                               long long* __restrict__ record, long long pixels) {
    const long long stride = (long long)gridDim.x * kBlock;
    int n_filled = 0, n_masked = 0;
    // the splat is complete: a valid pixel met exactly one of the four fates, and no launch adds to those words again
    if (blockIdx.x == 0 && threadIdx.x == 0)
        record[kValid] = ((record[kBehind] + record[kOutside]) + record[kEmptyRange]) + record[kWritten];
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < pixels; i += stride) {
        const unsigned bits = zbuffer[i];
        const bool filled = bits != kEmpty;
        const bool masked = colour_valid != nullptr && colour_valid[i] == 0;
        n_filled += filled ? 1 : 0;
        n_masked += filled && masked ? 1 : 0;
        out_depth[i] = filled && !masked ? __uint_as_float(bits) : 0.0f;
    }
    block_count_commit(n_filled, record + kFilled);
    block_count_commit(n_masked, record + kMasked);
}

__global__ __launch_bounds__(kBlock) void rgbd_rectify_kernel(const unsigned char* __restrict__ src,
                                                              unsigned char* __restrict__ dst,
                                                              unsigned char* __restrict__ valid, Lens l, Pinhole o,
                                                              int height, int width, int out_height, int out_width) {
    const long long total = (long long)out_height * out_width;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int v = (int)((unsigned)i / (unsigned)out_width), u = (int)(i - (long long)v * out_width);  // i < 2^31
        const double x = ((double)u - o.cx) / o.fx, y = ((double)v - o.cy) / o.fy;
        double xd, yd;
        distort(l, x, y, xd, yd);
        const double us = l.fx * xd + l.cx, vs = l.fy * yd + l.cy;
        // false for NaN; an infinity fails the upper bounds
        const bool ok = us >= 0.0 && us <= (double)(width - 1) && vs >= 0.0 && vs <= (double)(height - 1);
        unsigned char out[3] = {0, 0, 0};
        if (ok) {
            const double fu = floor(us), fv = floor(vs);
            const double a = us - fu, b = vs - fv;
            const int u0 = (int)fu, v0 = (int)fv;
            const int u1 = min(u0 + 1, width - 1), v1 = min(v0 + 1, height - 1);
            const unsigned char* r0 = src + ((long long)v0 * width) * 3;
            const unsigned char* r1 = src + ((long long)v1 * width) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double top = (double)r0[(long long)u0 * 3 + ch] * (1.0 - a) + (double)r0[(long long)u1 * 3 + ch] * a;
                const double bottom = (double)r1[(long long)u0 * 3 + ch] * (1.0 - a) + (double)r1[(long long)u1 * 3 + ch] * a;
                out[ch] = (unsigned char)floor((top * (1.0 - b) + bottom * b) + 0.5);
            }
        }
        dst[i * 3] = out[0];
        dst[i * 3 + 1] = out[1];
        dst[i * 3 + 2] = out[2];
        valid[i] = ok ? 1 : 0;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

bool is_finite(double v) { return v - v == 0.0; }

bool focal_ok(double f) { return is_finite(f) && f != 0.0; }

// the source camera of the ray table and of the rectified image
bool lens_of(const lsf_rgbd_params* q, Lens& l) {
    if (!focal_ok(q->fx) || !focal_ok(q->fy) || !is_finite(q->cx) || !is_finite(q->cy)) return false;
    bool zero = true;
    for (int j = 0; j < 8; ++j) {
        if (!is_finite(q->k[j])) return false;
        zero = zero && q->k[j] == 0.0;
    }
    l.fx = q->fx; l.fy = q->fy; l.cx = q->cx; l.cy = q->cy;
    l.k1 = q->k[0]; l.k2 = q->k[1]; l.p1 = q->k[2]; l.p2 = q->k[3];
    l.k3 = q->k[4]; l.k4 = q->k[5]; l.k5 = q->k[6]; l.k6 = q->k[7];
    l.pinhole = zero ? 1 : 0;
    return true;
}

bool output_of(const lsf_rgbd_params* q, Pinhole& o) {
    if (!focal_ok(q->out_fx) || !focal_ok(q->out_fy) || !is_finite(q->out_cx) || !is_finite(q->out_cy)) return false;
    o.fx = q->out_fx; o.fy = q->out_fy; o.cx = q->out_cx; o.cy = q->out_cy;
    return true;
}

int blocks_for(long long lanes) {
    const long long want = (lanes + kBlock - 1) / kBlock;
    return want > kMaxBlocks ? kMaxBlocks : (int)(want < 1 ? 1 : want);
}

struct Span {
    const void* at;
    size_t bytes;
};

template <int N>
bool any_overlap(const Span (&s)[N]) {
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j)
            if (overlaps(s[i].at, s[i].bytes, s[j].at, s[j].bytes)) return true;
    return false;
}

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

constexpr long long kMaxPixels = 0x7fffffffll;

}  // namespace

extern "C" int lsf_rgbd_ray_table(double* corner_rays, double* centre_rays, const lsf_rgbd_params* params,
                                  void* stream) {
    (void)hipGetLastError();
    if (!corner_rays || !centre_rays || !params) return LSF_ERR_BAD_ARGUMENT;
    if (params->height < 1 || params->width < 1) return LSF_ERR_BAD_ARGUMENT;
    Lens l;
    if (!lens_of(params, l)) return LSF_ERR_BAD_ARGUMENT;
    const long long corners = ((long long)params->height + 1) * ((long long)params->width + 1);
    if (corners > kMaxPixels) return LSF_ERR_BAD_DIMS;
    if (misaligned(corner_rays, 7) || misaligned(centre_rays, 7)) return LSF_ERR_BAD_ARGUMENT;
    const Span all[2] = {{corner_rays, (size_t)corners * 16},
                         {centre_rays, (size_t)params->height * params->width * 16}};
    if (any_overlap(all)) return LSF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(rgbd_ray_table_kernel, dim3(blocks_for(corners)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<double2*>(corner_rays), reinterpret_cast<double2*>(centre_rays), l,
                       params->height, params->width);
    return launch_status();
}

extern "C" int lsf_rgbd_register_depth(const void* depth, int32_t depth_dtype, const double* corner_rays,
                                       const double* centre_rays, uint32_t* zbuffer, const uint8_t* colour_valid,
                                       float* out_depth, int64_t* record, const lsf_rgbd_params* params, void* stream) {
    (void)hipGetLastError();
    if (!depth || !corner_rays || !centre_rays || !zbuffer || !out_depth || !record || !params)
        return LSF_ERR_BAD_ARGUMENT;
    if (!depth_dtype_ok(depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    const lsf_rgbd_params& q = *params;
    if (q.height < 1 || q.width < 1 || q.out_height < 1 || q.out_width < 1) return LSF_ERR_BAD_ARGUMENT;
    if (q.max_footprint < 1 || q.max_footprint > LSF_RGBD_MAX_FOOTPRINT) return LSF_ERR_BAD_ARGUMENT;
    Pinhole o;
    if (!output_of(params, o)) return LSF_ERR_BAD_ARGUMENT;
    Rigid g;
    for (int j = 0; j < 9; ++j) {
        if (!is_finite(q.rotation[j])) return LSF_ERR_BAD_ARGUMENT;
        g.r[j] = q.rotation[j];
    }
    for (int j = 0; j < 3; ++j) {
        if (!is_finite(q.translation[j])) return LSF_ERR_BAD_ARGUMENT;
        g.t[j] = q.translation[j];
    }
    if (!is_finite(q.depth_unit_ratio) || !(q.depth_unit_ratio > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    const long long corners = ((long long)q.height + 1) * ((long long)q.width + 1);
    const long long pixels = (long long)q.height * q.width, out_pixels = (long long)q.out_height * q.out_width;
    if (corners > kMaxPixels || out_pixels > kMaxPixels) return LSF_ERR_BAD_DIMS;
    const size_t depth_bytes = kDepthBytes[depth_dtype];
    if (misaligned(corner_rays, 7) || misaligned(centre_rays, 7) || misaligned(record, 7) || misaligned(zbuffer, 3) ||
        misaligned(out_depth, 3) || misaligned(depth, depth_bytes - 1))
        return LSF_ERR_BAD_ARGUMENT;
    const Span all[7] = {{depth, (size_t)pixels * depth_bytes}, {corner_rays, (size_t)corners * 16},
                         {centre_rays, (size_t)pixels * 16},   {zbuffer, (size_t)out_pixels * 4},
                         {colour_valid, (size_t)out_pixels},    {out_depth, (size_t)out_pixels * 4},
                         {record, (size_t)LSF_RGBD_RECORD_WORDS * 8}};
    if (any_overlap(all)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    long long* rec = reinterpret_cast<long long*>(record);
    hipLaunchKernelGGL(rgbd_clear_kernel, dim3(blocks_for(out_pixels)), dim3(kBlock), 0, s, zbuffer, rec, out_pixels);
    if (int e = launch_status()) return e;
    const double2* corner = reinterpret_cast<const double2*>(corner_rays);
    const double2* centre = reinterpret_cast<const double2*>(centre_rays);
    const int e = dispatch_depth(depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        hipLaunchKernelGGL(rgbd_splat_kernel<DT>, dim3(blocks_for(pixels)), dim3(kBlock), 0, s,
                           static_cast<const DT*>(depth), corner, centre, zbuffer, rec, g, o, q.depth_unit_ratio, q.height,
                           q.width, q.out_height, q.out_width, q.max_footprint);
        return launch_status();
    });
    if (e) return e;
    hipLaunchKernelGGL(rgbd_finalise_kernel, dim3(blocks_for(out_pixels)), dim3(kBlock), 0, s, zbuffer, colour_valid,
                       out_depth, rec, out_pixels);
    return launch_status();
}

extern "C" int lsf_rgbd_rectify_colour(const uint8_t* src, uint8_t* dst, uint8_t* valid, const lsf_rgbd_params* params,
                                       void* stream) {
    (void)hipGetLastError();
    if (!src || !dst || !valid || !params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_rgbd_params& q = *params;
    if (q.height < 1 || q.width < 1 || q.out_height < 1 || q.out_width < 1) return LSF_ERR_BAD_ARGUMENT;
    Lens l;
    Pinhole o;
    if (!lens_of(params, l) || !output_of(params, o)) return LSF_ERR_BAD_ARGUMENT;
    const long long pixels = (long long)q.height * q.width, out_pixels = (long long)q.out_height * q.out_width;
    if (pixels > kMaxPixels || out_pixels > kMaxPixels) return LSF_ERR_BAD_DIMS;
    const Span all[3] = {{src, (size_t)pixels * 3}, {dst, (size_t)out_pixels * 3}, {valid, (size_t)out_pixels}};
    if (any_overlap(all)) return LSF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(rgbd_rectify_kernel, dim3(blocks_for(out_pixels)), dim3(kBlock), 0, as_stream(stream), src, dst,
                       valid, l, o, q.height, q.width, q.out_height, q.out_width);
    return launch_status();
}
