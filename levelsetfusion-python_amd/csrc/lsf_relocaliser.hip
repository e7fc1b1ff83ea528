// Keyframe ferns for relocalisation (include/lsf_hip.h, lsf_reloc_encode / lsf_reloc_query; INTEGRATION.md section 3,
// "Tracking quality and relocalisation"; tests/relocaliser_restatement.py restates it): a depth (and colour) frame reduced
// to a coarse image of block means, the frame's fern code taken from that image, its distance to every stored keyframe,
// the nearest few, and the append of a frame that is far from all of them.
// Exactness.  A block mean is an INTEGER sum: a counting pixel adds q = rint(d * 2^20) (int64) and its three bytes, so the
// sum does not depend on the order and the shuffles below equal numpy's sum bit for bit; the one division per block is
// float64.  Everything else is comparisons and integer counts.  No float atomics, no atomics at all; no host wait.
// Shape.  Encode: a wave per coarse block, four blocks per workgroup; the lanes walk the block's pixels row-major, so a
// wave's loads are runs of the block's width (64 bytes of float32 at 640 x 480 with a 30 x 40 coarse image, the other half
// of each line being the neighbouring wave's), every byte of the frame read once.  A one-workgroup launch then sums the
// blocks' counts into the record.  Query: one launch rebuilds the frame's code (a lane per fern), one walks the database
// with a wave per keyframe row -- the frame's code in LDS, the row read as aligned 16-byte words whatever F is, the bytes
// outside the row masked -- and a last one-workgroup launch selects the nearest by (distance, id) and appends.
#include "lsf_tsdf_typed.h"

using namespace lsf;

namespace {

constexpr int kMaxBlocks = LSF_RELOC_MAX_BLOCKS;
constexpr int kMaxFerns = LSF_RELOC_MAX_FERNS;
constexpr int kMaxDecisions = LSF_RELOC_MAX_DECISIONS;
constexpr int kMaxCandidates = LSF_RELOC_MAX_CANDIDATES;
constexpr int kBlockWaves = kBlock / kWave;
constexpr double kQuantum = 1048576.0;  // 2^20
enum { kNBefore = 0, kIds = 1, kDistances = 5, kAppended = 9, kFull = 10 };
static_assert(kFull + 2 == LSF_RELOC_QUERY_RECORD_WORDS, "the query record's twelve words");

__device__ inline long long wave_sum(long long v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    return v;  // lane 0 holds the sum
}

// wave w of the grid takes coarse blocks w, w + waves, ...; lane 0 writes the block's C floats and its count
template <typename DT>
__global__ __launch_bounds__(kBlock) void reloc_encode_kernel(const DT* __restrict__ depth,
                                                              const unsigned char* __restrict__ colour,
                                                              float* __restrict__ coarse, int* __restrict__ block_counts,
                                                              double ratio, double near_m, double far_m, int height,
                                                              int width, int ch, int cw) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long waves = (long long)gridDim.x * kBlockWaves;
    const long long blocks = (long long)ch * cw;
    const int channels = colour != nullptr ? 4 : 1;
    for (long long b = (long long)blockIdx.x * kBlockWaves + threadIdx.x / kWave; b < blocks; b += waves) {
        const int bi = (int)(b / cw), bj = (int)(b - (long long)bi * cw);
        const int r0 = (int)((long long)bi * height / ch), r1 = (int)(((long long)bi + 1) * height / ch);
        const int c0 = (int)((long long)bj * width / cw), c1 = (int)(((long long)bj + 1) * width / cw);
        const int bw = c1 - c0;
        const long long pixels = (long long)(r1 - r0) * bw;
        long long sum_q = 0, count = 0, sum_r = 0, sum_g = 0, sum_b = 0;
        for (long long p = lane; p < pixels; p += kWave) {
            const int dr = (int)(p / bw), dc = (int)(p - (long long)dr * bw);
            const long long i = (long long)(r0 + dr) * width + (c0 + dc);
            const double d = (double)scaled_depth(depth, i, ratio);
            if (d >= near_m && d <= far_m) {  // false for NaN
                sum_q += (long long)rint(d * kQuantum);
                ++count;
                if (colour != nullptr) {
                    sum_r += colour[i * 3];
                    sum_g += colour[i * 3 + 1];
                    sum_b += colour[i * 3 + 2];
                }
            }
        }
        sum_q = wave_sum(sum_q);
        count = wave_sum(count);
        if (colour != nullptr) {
            sum_r = wave_sum(sum_r);
            sum_g = wave_sum(sum_g);
            sum_b = wave_sum(sum_b);
        }
        if (lane == 0) {
            const bool valid = 2 * count >= pixels;  // pixels >= 1, so a valid block has a counting pixel
            float* out = coarse + b * channels;
            out[0] = valid ? (float)(((double)sum_q / (double)count) / kQuantum) : 0.0f;
            if (colour != nullptr) {
                out[1] = valid ? (float)((double)sum_r / (double)count) : 0.0f;
                out[2] = valid ? (float)((double)sum_g / (double)count) : 0.0f;
                out[3] = valid ? (float)((double)sum_b / (double)count) : 0.0f;
            }
            block_counts[b] = (int)count;
        }
    }
}

// the workgroup's sum of a lane value, returned to thread 0: shuffles inside a wave, one LDS word per wave across them
__device__ inline long long block_sum(long long mine, long long* s_wave) {
    mine = wave_sum(mine);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = mine;
    __syncthreads();
    long long all = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlockWaves; ++w) all += s_wave[w];
    __syncthreads();
    return all;
}

// one workgroup: record = (counting pixels, valid blocks)
__global__ __launch_bounds__(kBlock) void reloc_encode_record_kernel(const float* __restrict__ coarse,
                                                                     const int* __restrict__ block_counts,
                                                                     int* __restrict__ record, long long blocks,
                                                                     int channels) {
    __shared__ long long s_wave[kBlockWaves];
    long long counting = 0, valid = 0;
    for (long long b = threadIdx.x; b < blocks; b += kBlock) {
        counting += block_counts[b];
        valid += coarse[b * channels] > 0.0f ? 1 : 0;
    }
    counting = block_sum(counting, s_wave);
    valid = block_sum(valid, s_wave);
    if (threadIdx.x == 0) {
        record[0] = (int)counting;
        record[1] = (int)valid;
    }
}

// a lane per fern: byte f of the frame's code, bit j from decision j.  A location or a channel outside the coarse image
// reads nothing and gives bit 0: the table is device data the host cannot check without waiting.
__global__ __launch_bounds__(kBlock) void reloc_code_kernel(const float* __restrict__ coarse,
                                                            const int* __restrict__ locations,
                                                            const unsigned char* __restrict__ channels,
                                                            const float* __restrict__ thresholds,
                                                            unsigned char* __restrict__ frame_code, int ferns,
                                                            int decisions, long long blocks, int coarse_channels) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= ferns) return;
    unsigned code = 0;
    for (int j = 0; j < decisions; ++j) {
        const long long at = (long long)f * decisions + j;
        const long long loc = locations[at];
        const int c = channels[at];
        if (loc < 0 || loc >= blocks || c >= coarse_channels) continue;
        const float value = coarse[loc * coarse_channels + c], d = coarse[loc * coarse_channels];
        if (value > thresholds[at] && d > 0.0f) code |= 1u << j;
    }
    frame_code[f] = (unsigned char)code;
}

// the database's size as the kernels read it: a value outside [0, capacity] cannot index the rows
__device__ inline int database_size(const int* n, int capacity) {
    const int v = *n;
    return v < 0 ? 0 : (v > capacity ? capacity : v);
}

// a wave per keyframe row k: the ferns whose byte differs from the frame's.  The row [k F, (k + 1) F) of the flat byte
// array is covered by aligned 16-byte words; a word that would reach past the array's end is read byte by byte.
__global__ __launch_bounds__(kBlock) void reloc_distance_kernel(const unsigned char* __restrict__ codes,
                                                                const unsigned char* __restrict__ frame_code,
                                                                const int* __restrict__ n_keyframes,
                                                                int* __restrict__ distances, int ferns, int capacity) {
    __shared__ unsigned char s_code[kMaxFerns];
    for (int i = threadIdx.x; i < ferns; i += kBlock) s_code[i] = frame_code[i];
    __syncthreads();
    const int n = database_size(n_keyframes, capacity);
    const int lane = threadIdx.x & (kWave - 1);
    const int waves = gridDim.x * kBlockWaves;
    const long long total = (long long)capacity * ferns;
    for (int k = blockIdx.x * kBlockWaves + threadIdx.x / kWave; k < capacity; k += waves) {
        if (k >= n) {  // uniform over the wave
            if (lane == 0) distances[k] = -1;
            continue;
        }
        const long long begin = (long long)k * ferns, end = begin + ferns;
        long long differing = 0;
        for (long long w = begin / 16 + lane; w * 16 < end; w += kWave) {
            const long long b0 = w * 16;
            unsigned char bytes[16];
            if (b0 + 16 <= total) {
                const uint4 v = *reinterpret_cast<const uint4*>(codes + b0);
                const unsigned word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 16; ++j) bytes[j] = (unsigned char)(word[j / 4] >> (8 * (j % 4)));
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) bytes[j] = b0 + j < total ? codes[b0 + j] : (unsigned char)0;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const long long at = b0 + j;
                if (at >= begin && at < end) differing += bytes[j] != s_code[at - begin] ? 1 : 0;
            }
        }
        differing = wave_sum(differing);
        if (lane == 0) distances[k] = (int)differing;
    }
}

// one workgroup: the `candidates` smallest keys (distance << 32 | id) in rising order, each the smallest key above the
// one before it; then the harvest rule, the append and the record
__global__ __launch_bounds__(kBlock) void reloc_select_kernel(unsigned char* __restrict__ codes,
                                                              const unsigned char* __restrict__ frame_code,
                                                              int* __restrict__ n_keyframes,
                                                              const int* __restrict__ distances, int* __restrict__ record,
                                                              int ferns, int capacity, int candidates, int harvest,
                                                              int harvest_differing) {
    __shared__ unsigned long long s_wave[kBlockWaves];
    __shared__ unsigned long long s_best;
    __shared__ int s_append;
    const unsigned long long none = ~0ull;
    const int n = database_size(n_keyframes, capacity);
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long previous = 0;
    int nearest = -1;  // thread 0: the smallest distance, -1 for an empty database
    for (int c = 0; c < kMaxCandidates; ++c) {
        unsigned long long best = none;
        if (c < candidates) {
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const unsigned long long key = ((unsigned long long)(unsigned)distances[k] << 32) | (unsigned)k;
                if ((c == 0 || key > previous) && key < best) best = key;
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const unsigned long long other = __shfl_down(best, d, kWave);
            best = other < best ? other : best;
        }
        if (lane == 0) s_wave[threadIdx.x / kWave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long all = none;
            for (int w = 0; w < kBlockWaves; ++w) all = s_wave[w] < all ? s_wave[w] : all;
            s_best = all;
            record[kIds + c] = all == none ? -1 : (int)(all & 0xffffffffull);
            record[kDistances + c] = all == none ? -1 : (int)(all >> 32);
            if (c == 0 && all != none) nearest = (int)(all >> 32);
        }
        __syncthreads();
        previous = s_best;
        if (previous == none) candidates = 0;  // nothing above the last key: the remaining slots are -1
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool wanted = harvest != 0 && (n == 0 || nearest >= harvest_differing);
        s_append = wanted && n < capacity ? 1 : 0;
        record[kNBefore] = n;
        record[kAppended] = s_append ? n : -1;
        record[kFull] = wanted && n >= capacity ? 1 : 0;
        record[kFull + 1] = 0;
    }
    __syncthreads();
    if (s_append) {  // n < capacity: the row lies inside the array
        unsigned char* row = codes + (long long)n * ferns;
        for (int i = threadIdx.x; i < ferns; i += kBlock) row[i] = frame_code[i];
        if (threadIdx.x == 0) *n_keyframes = n + 1;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

bool is_finite(double v) { return v - v == 0.0; }

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

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

constexpr long long kMaxIndex = 0x7fffffffll;

// the coarse image's extents and channels: what both entry points read
bool coarse_ok(const lsf_reloc_params& q) {
    if (q.coarse_height < 1 || q.coarse_width < 1) return false;
    if (q.channels != 1 && q.channels != 4) return false;
    return (long long)q.coarse_height * q.coarse_width * q.channels <= kMaxIndex;
}

int blocks_for(long long waves) {
    const long long want = (waves + kBlockWaves - 1) / kBlockWaves;
    return want > kMaxBlocks ? kMaxBlocks : (int)(want < 1 ? 1 : want);
}

}  // namespace

extern "C" int lsf_reloc_encode(const void* depth, int32_t depth_dtype, const uint8_t* colour, float* coarse,
                                int32_t* block_counts, int32_t* record, const lsf_reloc_params* params, void* stream) {
    (void)hipGetLastError();
    if (!depth || !coarse || !block_counts || !record || !params) return LSF_ERR_BAD_ARGUMENT;
    if (!depth_dtype_ok(depth_dtype)) return LSF_ERR_BAD_ARGUMENT;
    const lsf_reloc_params& q = *params;
    if (q.height < 1 || q.width < 1 || !coarse_ok(q)) return LSF_ERR_BAD_ARGUMENT;
    if (q.coarse_height > q.height || q.coarse_width > q.width) return LSF_ERR_BAD_ARGUMENT;
    if (q.channels != (colour ? 4 : 1)) return LSF_ERR_BAD_ARGUMENT;
    if (!is_finite(q.depth_unit_ratio) || !(q.depth_unit_ratio > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    if (!is_finite(q.depth_near) || !is_finite(q.depth_far) || !(q.depth_near > 0.0) || !(q.depth_near < q.depth_far) ||
        !(q.depth_far <= LSF_RELOC_MAX_DEPTH))
        return LSF_ERR_BAD_ARGUMENT;
    const long long pixels = (long long)q.height * q.width;
    if (pixels > kMaxIndex) return LSF_ERR_BAD_DIMS;
    const long long blocks = (long long)q.coarse_height * q.coarse_width;
    const size_t depth_bytes = kDepthBytes[depth_dtype];
    if (misaligned(depth, depth_bytes - 1) || misaligned(coarse, 3) || misaligned(block_counts, 3) ||
        misaligned(record, 3))
        return LSF_ERR_BAD_ARGUMENT;
    const Span all[5] = {{depth, (size_t)pixels * depth_bytes},
                         {colour, (size_t)pixels * 3},
                         {coarse, (size_t)blocks * q.channels * 4},
                         {block_counts, (size_t)blocks * 4},
                         {record, (size_t)LSF_RELOC_ENCODE_RECORD_WORDS * 4}};
    if (any_overlap(all)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const int e = dispatch_depth(depth_dtype, [&](auto dt) {
        using DT = decltype(dt);
        hipLaunchKernelGGL(reloc_encode_kernel<DT>, dim3(blocks_for(blocks)), dim3(kBlock), 0, s,
                           static_cast<const DT*>(depth), colour, coarse, block_counts, q.depth_unit_ratio, q.depth_near, q.depth_far,
                           q.height, q.width, q.coarse_height, q.coarse_width);
        return launch_status();
    });
    if (e) return e;
    hipLaunchKernelGGL(reloc_encode_record_kernel, dim3(1), dim3(kBlock), 0, s, coarse, block_counts, record, blocks,
                       q.channels);
    return launch_status();
}

extern "C" int lsf_reloc_query(const float* coarse, const int32_t* locations, const uint8_t* channels,
                               const float* thresholds, uint8_t* codes, int32_t* n_keyframes, uint8_t* frame_code,
                               int32_t* distances, int32_t* record, const lsf_reloc_params* params, void* stream) {
    (void)hipGetLastError();
    if (!coarse || !locations || !channels || !thresholds || !codes || !n_keyframes || !frame_code || !distances ||
        !record || !params)
        return LSF_ERR_BAD_ARGUMENT;
    const lsf_reloc_params& q = *params;
    if (!coarse_ok(q)) return LSF_ERR_BAD_ARGUMENT;
    if (q.ferns < 1 || q.ferns > kMaxFerns || q.decisions < 1 || q.decisions > kMaxDecisions)
        return LSF_ERR_BAD_ARGUMENT;
    if (q.candidates < 1 || q.candidates > kMaxCandidates || q.capacity < 1) return LSF_ERR_BAD_ARGUMENT;
    if (q.harvest != 0 && q.harvest != 1) return LSF_ERR_BAD_ARGUMENT;
    if (q.harvest && q.harvest_differing < 1) return LSF_ERR_BAD_ARGUMENT;
    const long long database = (long long)q.capacity * q.ferns;
    if (database > kMaxIndex) return LSF_ERR_BAD_DIMS;
    if (misaligned(coarse, 3) || misaligned(locations, 3) || misaligned(thresholds, 3) || misaligned(codes, 15) ||
        misaligned(n_keyframes, 3) || misaligned(distances, 3) || misaligned(record, 3))
        return LSF_ERR_BAD_ARGUMENT;
    const long long blocks = (long long)q.coarse_height * q.coarse_width;
    const size_t table = (size_t)q.ferns * q.decisions;
    const Span all[9] = {{coarse, (size_t)blocks * q.channels * 4},
                         {locations, table * 4},
                         {channels, table},
                         {thresholds, table * 4},
                         {codes, (size_t)database},
                         {n_keyframes, 4},
                         {frame_code, (size_t)q.ferns},
                         {distances, (size_t)q.capacity * 4},
                         {record, (size_t)LSF_RELOC_QUERY_RECORD_WORDS * 4}};
    if (any_overlap(all)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(reloc_code_kernel, dim3((q.ferns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, coarse, locations,
                       channels, thresholds, frame_code, q.ferns, q.decisions, blocks, q.channels);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(reloc_distance_kernel, dim3(blocks_for(q.capacity)), dim3(kBlock), 0, s, codes, frame_code,
                       n_keyframes, distances, q.ferns, q.capacity);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(reloc_select_kernel, dim3(1), dim3(kBlock), 0, s, codes, frame_code, n_keyframes, distances,
                       record, q.ferns, q.capacity, q.candidates, q.harvest, q.harvest_differing);
    return launch_status();
}
