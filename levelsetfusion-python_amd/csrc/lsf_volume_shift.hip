// The moving volume's shifted copy (include/lsf_hip.h, lsf_volume_shift; INTEGRATION.md section 3, "Moving volume";
// tests/volume_shift_restatement.py restates it): out of place, one launch,
//     dst(v) = src(v + s) where v + s lies inside the volume, else (tsdf 1, weight 0, colour record 0 0 0 0).
// Values move as 32-bit words: nothing is computed, so NaN payloads and -0.0 survive.
// A pure stream, so the shape is decided by the memory system alone.  The unit of work is one destination ROW (z, y):
// whether its source row (z + sz, y + sy) exists is one wave-uniform decision, the row's retained x range is the same
// for every row, and no voxel index is divided.  A wave owns a row; the four waves of a workgroup own four consecutive
// rows, and the grid is capped (LSF_VOLUME_SHIFT_MAX_BLOCKS: eight workgroups per CU) with a stride loop behind it, so
// a 512^3 volume (262144 rows) runs on 2048 workgroups.
// Access widths.  tsdf and weight move four voxels per lane.  A destination row starts at (z ny + y) nx and its source at
// that plus a multiple of nx plus shift_x, so with shift_x % 4 != 0 the two sides can never both be 16-byte aligned.
// Global dwordx4 accesses need dword alignment only on gfx950, so both sides keep the 16-byte width and the four-voxel
// groups are anchored at the DESTINATION row's start: a wave-instruction writes one contiguous KiB and reads one
// contiguous KiB displaced by shift_x words.  profiles/moving_volume_cost.md has the measured price of the displaced read.
// A group that straddles an end of the retained range is loaded word by word and stored as one group; the nx % 4 voxels
// at a row's end are stored word by word.  The colour record is one 16-byte load and one 16-byte store per lane, four
// records in flight per lane.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kMaxBlocks = LSF_VOLUME_SHIFT_MAX_BLOCKS;
constexpr int kRowsPerBlock = kBlock / kWave;
static_assert(kRowsPerBlock == LSF_VOLUME_SHIFT_BLOCK_ROWS, "a wave per row");
constexpr unsigned kTsdfFill = 0x3f800000u;  // 1.0f
constexpr unsigned kWeightFill = 0u;
constexpr int kColourInFlight = 4;

// four voxels of a row as one 16-byte access at dword alignment
struct __attribute__((packed, aligned(4))) Quad {
    unsigned v[4];
};

struct ShiftDev {
    int nx, ny, nz;
    int sx, sy, sz;       // clamped to [-n, n] per axis
    int x_lo, x_hi;       // the destination x whose source x + sx lies inside a row: [x_lo, x_hi), empty when x_lo >= x_hi
    long long rows;       // nz * ny
    int nblocks;
};

// one scalar plane (tsdf or weight) of one destination row.  src_row / dst_row: the rows' first words; src_row is
// already displaced by sx and is only dereferenced for x in [x_lo, x_hi).
__device__ inline void shift_row(const unsigned* __restrict__ src_row, unsigned* __restrict__ dst_row, bool row_kept,
                                 unsigned fill, int lane, const ShiftDev& p) {
    const int lo = row_kept ? p.x_lo : 0, hi = row_kept ? p.x_hi : 0;
    for (int x = lane * 4; x < p.nx; x += kWave * 4) {
        // the loads of both branches are in flight before the first store waits for them
        Quad q = {{fill, fill, fill, fill}};
        if (x >= lo && x + 4 <= hi) {
            q = *reinterpret_cast<const Quad*>(src_row + x);
        } else {  // a group across an end of the retained range (hi <= nx), or outside it
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k >= lo && x + k < hi) q.v[k] = src_row[x + k];
        }
        if (x + 4 <= p.nx) {
            *reinterpret_cast<Quad*>(dst_row + x) = q;
        } else {  // the nx % 4 voxels at the row's end
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < p.nx) dst_row[x + k] = q.v[k];
        }
    }
}

template <bool COLOUR>
__global__ __launch_bounds__(kBlock) void volume_shift_kernel(const unsigned* __restrict__ tsdf,
                                                              const unsigned* __restrict__ weight,
                                                              const uint4* __restrict__ colour,
                                                              unsigned* __restrict__ out_tsdf,
                                                              unsigned* __restrict__ out_weight,
                                                              uint4* __restrict__ out_colour, ShiftDev p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    for (long long row = (long long)blockIdx.x * kRowsPerBlock + wave; row < p.rows; row += stride) {
        const int z = (int)(row / p.ny), y = (int)(row - (long long)z * p.ny);
        const int zs = z + p.sz, ys = y + p.sy;  // |s| <= n: no overflow
        const bool row_kept = (unsigned)zs < (unsigned)p.nz && (unsigned)ys < (unsigned)p.ny;
        const long long dst_at = row * p.nx;
        // the source row's first word, displaced by sx; never formed into an address when the row leaves
        const long long src_at = row_kept ? ((long long)zs * p.ny + ys) * p.nx + p.sx : 0;
        shift_row(tsdf + src_at, out_tsdf + dst_at, row_kept, kTsdfFill, lane, p);
        shift_row(weight + src_at, out_weight + dst_at, row_kept, kWeightFill, lane, p);
        if (COLOUR) {
            const uint4* __restrict__ src_row = colour + src_at;
            uint4* __restrict__ dst_row = out_colour + dst_at;
            const int lo = row_kept ? p.x_lo : 0, hi = row_kept ? p.x_hi : 0;
            for (int x = lane; x < p.nx; x += kWave * kColourInFlight) {
                uint4 c[kColourInFlight];
#pragma unroll
                for (int k = 0; k < kColourInFlight; ++k) {
                    const int xk = x + k * kWave;
                    c[k] = make_uint4(0u, 0u, 0u, 0u);
                    if (xk >= lo && xk < hi) c[k] = src_row[xk];  // hi <= nx
                }
#pragma unroll
                for (int k = 0; k < kColourInFlight; ++k) {
                    const int xk = x + k * kWave;
                    if (xk < p.nx) dst_row[xk] = c[k];
                }
            }
        }
    }
}

int clamp_shift(int s, int n) { return s < -n ? -n : (s > n ? n : s); }

int convert(const lsf_volume_shift_params* q, ShiftDev& p) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->depth < 1 || q->height < 1 || q->width < 1) return LSF_ERR_BAD_ARGUMENT;
    p.rows = (long long)q->depth * q->height;
    if (p.rows * q->width > 0x7fffffffll) return LSF_ERR_BAD_DIMS;
    p.nx = q->width; p.ny = q->height; p.nz = q->depth;
    p.sx = clamp_shift(q->shift_x, p.nx);
    p.sy = clamp_shift(q->shift_y, p.ny);
    p.sz = clamp_shift(q->shift_z, p.nz);
    p.x_lo = p.sx < 0 ? -p.sx : 0;
    p.x_hi = p.sx > 0 ? p.nx - p.sx : p.nx;
    const long long want = (p.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    p.nblocks = want > kMaxBlocks ? kMaxBlocks : (int)want;
    return 0;
}

// no output overlaps an input or another output
template <int NI, int NO>
bool any_alias(const void* const (&ins)[NI], const size_t (&in_bytes)[NI], const void* const (&outs)[NO],
               const size_t (&out_bytes)[NO]) {
    for (int i = 0; i < NO; ++i) {
        for (int j = 0; j < NI; ++j)
            if (overlaps(outs[i], out_bytes[i], ins[j], in_bytes[j])) return true;
        for (int j = i + 1; j < NO; ++j)
            if (overlaps(outs[i], out_bytes[i], outs[j], out_bytes[j])) return true;
    }
    return false;
}

}  // namespace

extern "C" int lsf_volume_shift(const float* tsdf, const float* weight, const float* colour, float* out_tsdf,
                                float* out_weight, float* out_colour, const lsf_volume_shift_params* params,
                                void* stream) {
    (void)hipGetLastError();
    ShiftDev p;
    if (int e = convert(params, p)) return e;
    if (!tsdf || !weight || !out_tsdf || !out_weight || tsdf == weight) return LSF_ERR_BAD_ARGUMENT;
    if ((colour == nullptr) != (out_colour == nullptr)) return LSF_ERR_BAD_ARGUMENT;
    const uintptr_t words = (uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)out_tsdf | (uintptr_t)out_weight;
    if ((words & 3) != 0) return LSF_ERR_BAD_ARGUMENT;
    if ((((uintptr_t)colour | (uintptr_t)out_colour) & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.rows * (size_t)p.nx;
    const void* const ins[3] = {tsdf, weight, colour};
    const size_t in_bytes[3] = {n * 4, n * 4, n * 16};
    const void* const outs[3] = {out_tsdf, out_weight, out_colour};
    const size_t out_bytes[3] = {n * 4, n * 4, n * 16};
    if (any_alias(ins, in_bytes, outs, out_bytes)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const unsigned* t = reinterpret_cast<const unsigned*>(tsdf);
    const unsigned* w = reinterpret_cast<const unsigned*>(weight);
    unsigned* ot = reinterpret_cast<unsigned*>(out_tsdf);
    unsigned* ow = reinterpret_cast<unsigned*>(out_weight);
    if (colour)
        hipLaunchKernelGGL(volume_shift_kernel<true>, dim3(p.nblocks), dim3(kBlock), 0, s, t, w,
                           reinterpret_cast<const uint4*>(colour), ot, ow, reinterpret_cast<uint4*>(out_colour), p);
    else
        hipLaunchKernelGGL(volume_shift_kernel<false>, dim3(p.nblocks), dim3(kBlock), 0, s, t, w,
                           (const uint4*)nullptr, ot, ow, (uint4*)nullptr, p);
    return launch_status();
}
