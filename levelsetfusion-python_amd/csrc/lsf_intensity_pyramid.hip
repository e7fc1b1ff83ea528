// The intensity pyramids of photometric ICP over the depth pyramid (include/lsf_hip.h, lsf_intensity_pyramid): one for
// the live colour image, one for the ray-cast prediction's Y channel.  The arithmetic is INTEGRATION.md section 3
// ("Intensity pyramid"); tests/pyramid_photometric_restatement.py restates it.  Every per-pixel step is one float64
// operation in the order written there, and -ffp-contract=off keeps products and sums separately rounded, so every
// level equals the restatement bit for bit.  `levels` launches, back to back, one lane per output pixel:
//   level 0    the source's intensity: Y of the pixel's three bytes, or the prediction's fourth channel copied
//   downsample level l + 1 from level l: the mean of the 2 x 2 block, NaN when one of the four is not finite
#include "lsf_device.h"

using namespace lsf;

namespace {

// Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 of a uint8 [n][3] image, photometric ICP's live intensity
__global__ __launch_bounds__(kBlock) void luminance_kernel(const uint8_t* __restrict__ image, float* __restrict__ out,
                                                           long long n) {
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= n) return;
    const uint8_t* c = image + at * 3;
    out[at] = (float)(((0.299 * (double)c[0] + 0.587 * (double)c[1]) + 0.114 * (double)c[2]) / 255.0);
}

// channel 3 of a float32 [n][4] image, moved as 32-bit words: a NaN keeps its bits
__global__ __launch_bounds__(kBlock) void channel_kernel(const uint32_t* __restrict__ image,
                                                         uint32_t* __restrict__ out, long long n) {
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= n) return;
    out[at] = image[at * 4 + 3];
}

// level l + 1 (extents h x w) from level l (row length w_in): ((q00 + q10) + (q01 + q11)) / 4, NaN unless all four
// are finite -- a surface's intensity is never mixed with "no colour"
__global__ __launch_bounds__(kBlock) void downsample_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int h, int w, int w_in) {
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= (long long)h * w) return;
    const int i = (int)(at / w), j = (int)(at % w);
    const float* q = in + (long long)(2 * i) * w_in + 2 * j;
    const double q00 = (double)q[0], q10 = (double)q[1], q01 = (double)q[w_in], q11 = (double)q[w_in + 1];
    float value = NAN;
    if (isfinite(q00) && isfinite(q10) && isfinite(q01) && isfinite(q11))
        value = (float)(((q00 + q10) + (q01 + q11)) / 4.0);
    out[at] = value;
}

unsigned blocks_of(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int lsf_intensity_pyramid(const void* image, float* pyramid_intensity,
                                     const lsf_intensity_pyramid_params* params, void* stream) {
    (void)hipGetLastError();
    if (!image || !pyramid_intensity || !params) return LSF_ERR_BAD_ARGUMENT;
    const lsf_intensity_pyramid_params* q = params;
    if (q->height < 1 || q->width < 1 || (long long)q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    if (q->levels < 1 || q->levels > LSF_ICP_MAX_LEVELS || (q->height >> (q->levels - 1)) < 1 ||
        (q->width >> (q->levels - 1)) < 1)
        return LSF_ERR_BAD_ARGUMENT;
    if (q->source != LSF_INTENSITY_SOURCE_COLOUR && q->source != LSF_INTENSITY_SOURCE_PREDICTION)
        return LSF_ERR_BAD_ARGUMENT;
    long long offset[LSF_ICP_MAX_LEVELS + 1] = {0};  // level l's first pixel; offset[levels] = the pyramid's pixels
    for (int l = 0; l < q->levels; ++l) offset[l + 1] = offset[l] + (long long)(q->height >> l) * (q->width >> l);
    const long long n = offset[1];
    const size_t in_bytes = (size_t)n * (q->source == LSF_INTENSITY_SOURCE_COLOUR ? 3 : 16);
    if (overlaps(image, in_bytes, pyramid_intensity, (size_t)offset[q->levels] * 4)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    if (q->source == LSF_INTENSITY_SOURCE_COLOUR)
        hipLaunchKernelGGL(luminance_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s,
                           reinterpret_cast<const uint8_t*>(image), pyramid_intensity, n);
    else
        hipLaunchKernelGGL(channel_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, s,
                           reinterpret_cast<const uint32_t*>(image), reinterpret_cast<uint32_t*>(pyramid_intensity), n);
    int e = launch_status();
    for (int l = 1; l < q->levels && e == 0; ++l) {
        const int h = q->height >> l, w = q->width >> l;
        hipLaunchKernelGGL(downsample_kernel, dim3(blocks_of((long long)h * w)), dim3(kBlock), 0, s,
                           pyramid_intensity + offset[l - 1], pyramid_intensity + offset[l], h, w, q->width >> (l - 1));
        e = launch_status();
    }
    return e;
}
