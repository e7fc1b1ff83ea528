// The moving volume's brick store on the card (include/lsf_hip.h, lsf_volume_bricks_count / _gather / _scatter;
// INTEGRATION.md section 3, "Brick store"; tests/volume_bricks_restatement.py restates it): what leaves the window with
// data in it is compacted into 8^3 bricks on an integer lattice, and what re-enters is written back in place.
// The window's voxel v is lattice voxel g + v; a brick's voxel (0, 0, 0) sits at window coordinate w0 = 8 b - g, which is
// negative or runs past n on the bricks the window's faces cut.  lsf_volume_shift makes dst(v) = src(v + s): a voxel u of
// the OLD window leaves when u - s lies outside the volume, a voxel v of the NEW window entered when v + s does (s
// clamped to [-n, n]).  Either way a voxel is OUT when, on some axis, it lies outside a retained range [k_lo, k_hi);
// the two differ in the sign of s only, so one predicate serves all three kernels.
// Shape.  One wave owns one brick, lane r the x-row (zl, yl) = (r / 8, r % 8): 8 consecutive words of tsdf and of weight.
// Whether a brick holds an OUT voxel at all follows from w0 and the retained ranges alone, a wave-uniform test before any
// load: a shift by a few voxels touches a shell of bricks and the rest of the grid costs one scalar decision each.  A row
// whose 8 voxels are all inside the window moves as two 16-byte accesses at dword alignment (gfx950 asks no more of a
// global dwordx4; lsf_volume_shift.hip's Quad), anything else word by word.  The flag of a brick is one ballot; the
// validity byte is the lane's own.  Four bricks per workgroup, a capped grid with a stride loop behind it.  The prefix sum
// of the flags is a single workgroup's (the grid has one int per 512 voxels), so the order of the rows is the grid's
// whatever the schedule, and nothing waits on another workgroup.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kBrick = LSF_VOLUME_BRICK;
constexpr int kBrickVoxels = kBrick * kBrick * kBrick;
constexpr int kMaxBlocks = LSF_VOLUME_BRICKS_MAX_BLOCKS;
constexpr int kBricksPerBlock = kBlock / kWave;
static_assert(kBricksPerBlock == LSF_VOLUME_BRICKS_BLOCK_BRICKS, "a wave per brick");
static_assert(kBrick * kBrick == kWave, "a lane per x-row of a brick");
constexpr int kScanBlock = 1024;
constexpr int kScanItems = 8;  // flags per thread and trip of the scan
constexpr unsigned kTsdfFill = 0x3f800000u;  // 1.0f
constexpr unsigned kDataBits = 0x7fffffffu;  // a weight holds data when any of these is set

// four voxels of a row as one 16-byte access at dword alignment
struct __attribute__((packed, aligned(4))) Quad {
    unsigned v[4];
};

struct BricksDev {
    int nx, ny, nz;
    int gx, gy, gz;
    int lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;  // the retained range per axis (convert: of the old or of the new window)
    int bx0, by0, bz0;                       // the grid's first brick
    int nbx, nby, nbz;
    int nbricks;
};

__host__ __device__ inline int floor_div8(int a) { return a >> 3; }  // arithmetic shift: floor for negative a too

// a brick of the grid: the window coordinate of its voxel (0, 0, 0), and whether any of its voxels inside the window is OUT
struct BrickAt {
    int x0, y0, z0;
    bool touches;
};

__device__ inline bool axis_out(int w0, int n, int lo, int hi) {
    const int a = max(w0, 0), e = min(w0 + kBrick, n);  // the brick's voxels inside the window, [a, e)
    return a < lo || e > hi;
}

__device__ inline BrickAt brick_at(int bx, int by, int bz, const BricksDev& p) {
    BrickAt b;
    b.x0 = bx * kBrick - p.gx;
    b.y0 = by * kBrick - p.gy;
    b.z0 = bz * kBrick - p.gz;
    b.touches = axis_out(b.x0, p.nx, p.lo_x, p.hi_x) || axis_out(b.y0, p.ny, p.lo_y, p.hi_y) ||
                axis_out(b.z0, p.nz, p.lo_z, p.hi_z);
    return b;
}

__device__ inline void grid_brick(int b, const BricksDev& p, int& bx, int& by, int& bz) {
    const int zy = b / p.nbx;
    bx = p.bx0 + (b - zy * p.nbx);
    bz = zy / p.nby;
    by = p.by0 + (zy - bz * p.nby);
    bz += p.bz0;
}

// the lane's row of a brick: its first word in the window (valid only where a voxel is inside), whether all 8 voxels
// are inside, and the bit mask of the voxels that are inside the window AND out of the retained box
struct Row {
    long long at;
    bool whole;
    unsigned out_mask;
};

__device__ inline Row lane_row(const BrickAt& b, int lane, const BricksDev& p) {
    const int z = b.z0 + (lane >> 3), y = b.y0 + (lane & 7);
    const bool row_in = (unsigned)z < (unsigned)p.nz && (unsigned)y < (unsigned)p.ny;
    const bool row_out = z < p.lo_z || z >= p.hi_z || y < p.lo_y || y >= p.hi_y;
    Row r;
    r.at = row_in ? ((long long)z * p.ny + y) * p.nx + b.x0 : 0;
    r.whole = row_in && b.x0 >= 0 && b.x0 + kBrick <= p.nx;
    r.out_mask = 0u;
#pragma unroll
    for (int k = 0; k < kBrick; ++k) {
        const int x = b.x0 + k;
        const bool in = row_in && (unsigned)x < (unsigned)p.nx;
        const bool out = row_out || x < p.lo_x || x >= p.hi_x;
        r.out_mask |= (in && out) ? (1u << k) : 0u;
    }
    return r;
}

// the 8 words of a window row; word k is read only when bit k of `want` is set (those voxels are inside the window)
__device__ inline void load_row(const unsigned* __restrict__ src, const Row& r, unsigned want, unsigned fill,
                                unsigned (&w)[kBrick]) {
#pragma unroll
    for (int k = 0; k < kBrick; ++k) w[k] = fill;
    if (want == 0u) return;
    if (r.whole) {
        const Quad a = *reinterpret_cast<const Quad*>(src + r.at);
        const Quad b = *reinterpret_cast<const Quad*>(src + r.at + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = a.v[k];
            w[k + 4] = b.v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < kBrick; ++k)
            if (want >> k & 1u) w[k] = src[r.at + k];
    }
}

// the voxels of the lane's row that are inside the window, OUT and hold data
__device__ inline unsigned data_mask(const unsigned* __restrict__ weight, const Row& r, unsigned (&w)[kBrick]) {
    load_row(weight, r, r.out_mask, 0u, w);
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < kBrick; ++k) m |= (w[k] & kDataBits) != 0u ? (1u << k) : 0u;
    return m & r.out_mask;
}

__global__ __launch_bounds__(kBlock) void bricks_flag_kernel(const unsigned* __restrict__ weight,
                                                             int* __restrict__ flags, BricksDev p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int stride = gridDim.x * kBricksPerBlock;
    for (int b = blockIdx.x * kBricksPerBlock + wave; b < p.nbricks; b += stride) {
        int bx, by, bz;
        grid_brick(b, p, bx, by, bz);
        const BrickAt at = brick_at(bx, by, bz, p);
        int flag = 0;
        if (at.touches) {  // wave-uniform
            const Row r = lane_row(at, lane, p);
            unsigned w[kBrick];
            flag = __ballot(data_mask(weight, r, w) != 0u) != 0ull ? 1 : 0;
        }
        if (lane == 0) flags[b] = flag;
    }
}

// exclusive prefix sum of n flags and their total, one workgroup: 8192 at a time (8 consecutive flags per thread, two
// 16-byte accesses each way) with the running sum carried along
__global__ __launch_bounds__(kScanBlock) void bricks_scan_kernel(const int* __restrict__ flags, int* __restrict__ offsets,
                                                                 long long* __restrict__ total, int n) {
    __shared__ int s_wave[kScanBlock / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    long long carry = 0;
    for (long long base = 0; base < n; base += kScanBlock * kScanItems) {
        const long long i0 = base + (long long)tid * kScanItems;
        const bool whole = i0 + kScanItems <= n;
        int f[kScanItems];
        if (whole) {
            const Quad a = *reinterpret_cast<const Quad*>(flags + i0);
            const Quad b = *reinterpret_cast<const Quad*>(flags + i0 + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f[k] = (int)a.v[k];
                f[k + 4] = (int)b.v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; ++k) f[k] = i0 + k < n ? flags[i0 + k] : 0;
        }
        int mine = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {  // f becomes the exclusive prefix inside the thread
            const int t = f[k];
            f[k] = mine;
            mine += t;
        }
        int v = mine;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(v, d, kWave);
            if (lane >= d) v += o;
        }
        if (lane == kWave - 1) s_wave[wave] = v;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kScanBlock / kWave; ++k) {
            const int t = s_wave[k];
            before += k < wave ? t : 0;
            all += t;
        }
        const int first = (int)(carry + before + v - mine);
        if (whole) {
            Quad a, b;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a.v[k] = (unsigned)(first + f[k]);
                b.v[k] = (unsigned)(first + f[k + 4]);
            }
            *reinterpret_cast<Quad*>(offsets + i0) = a;
            *reinterpret_cast<Quad*>(offsets + i0 + 4) = b;
        } else {
#pragma unroll
            for (int k = 0; k < kScanItems; ++k)
                if (i0 + k < n) offsets[i0 + k] = first + f[k];
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

template <bool COLOUR>
__global__ __launch_bounds__(kBlock) void bricks_gather_kernel(
    const unsigned* __restrict__ tsdf, const unsigned* __restrict__ weight, const uint4* __restrict__ colour,
    const int* __restrict__ flags, const int* __restrict__ offsets, long long brick_count, int* __restrict__ out_coords,
    unsigned* __restrict__ out_tsdf, unsigned* __restrict__ out_weight, uint4* __restrict__ out_colour,
    unsigned char* __restrict__ out_valid, BricksDev p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int stride = gridDim.x * kBricksPerBlock;
    for (int b = blockIdx.x * kBricksPerBlock + wave; b < p.nbricks; b += stride) {
        int bx, by, bz;
        grid_brick(b, p, bx, by, bz);
        const BrickAt at = brick_at(bx, by, bz, p);
        if (!at.touches) continue;  // never flagged
        if (__builtin_amdgcn_readfirstlane(flags[b]) == 0) continue;
        const long long slot = __builtin_amdgcn_readfirstlane(offsets[b]);
        if (slot < 0 || slot >= brick_count) continue;  // never with lsf_volume_bricks_count's own outputs
        const Row r = lane_row(at, lane, p);
        unsigned w[kBrick], t[kBrick];
        const unsigned valid = data_mask(weight, r, w);
        load_row(tsdf, r, valid, kTsdfFill, t);
        Quad qt[2], qw[2];
#pragma unroll
        for (int k = 0; k < kBrick; ++k) {
            const bool keep = valid >> k & 1u;
            qt[k >> 2].v[k & 3] = keep ? t[k] : kTsdfFill;
            qw[k >> 2].v[k & 3] = keep ? w[k] : 0u;
        }
        const long long row = slot * kBrickVoxels + lane * kBrick;
        *reinterpret_cast<Quad*>(out_tsdf + row) = qt[0];
        *reinterpret_cast<Quad*>(out_tsdf + row + 4) = qt[1];
        *reinterpret_cast<Quad*>(out_weight + row) = qw[0];
        *reinterpret_cast<Quad*>(out_weight + row + 4) = qw[1];
        out_valid[slot * kWave + lane] = (unsigned char)valid;
        if (lane < 3) out_coords[slot * 3 + lane] = lane == 0 ? bx : (lane == 1 ? by : bz);
        if (COLOUR) {
            uint4 c[kBrick];
#pragma unroll
            for (int k = 0; k < kBrick; ++k) {
                c[k] = make_uint4(0u, 0u, 0u, 0u);
                if (valid >> k & 1u) c[k] = colour[r.at + k];
            }
#pragma unroll
            for (int k = 0; k < kBrick; ++k) out_colour[row + k] = c[k];
        }
    }
}

template <bool COLOUR>
__global__ __launch_bounds__(kBlock) void bricks_scatter_kernel(
    const int* __restrict__ coords, const unsigned* __restrict__ brick_tsdf, const unsigned* __restrict__ brick_weight,
    const uint4* __restrict__ brick_colour, const unsigned char* __restrict__ brick_valid, long long brick_count,
    unsigned* __restrict__ tsdf, unsigned* __restrict__ weight, uint4* __restrict__ colour, BricksDev p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const long long stride = (long long)gridDim.x * kBricksPerBlock;
    for (long long k = (long long)blockIdx.x * kBricksPerBlock + wave; k < brick_count; k += stride) {
        const int bx = __builtin_amdgcn_readfirstlane(coords[k * 3]);
        const int by = __builtin_amdgcn_readfirstlane(coords[k * 3 + 1]);
        const int bz = __builtin_amdgcn_readfirstlane(coords[k * 3 + 2]);
        // outside the window's grid: skipped, before 8 b - g is formed
        if (bx < p.bx0 || bx >= p.bx0 + p.nbx || by < p.by0 || by >= p.by0 + p.nby || bz < p.bz0 || bz >= p.bz0 + p.nbz)
            continue;
        const BrickAt at = brick_at(bx, by, bz, p);
        if (!at.touches) continue;
        const Row r = lane_row(at, lane, p);
        const unsigned take = r.out_mask & (unsigned)brick_valid[k * kWave + lane];
        if (take == 0u) continue;
        const long long row = k * kBrickVoxels + lane * kBrick;
        const Quad t0 = *reinterpret_cast<const Quad*>(brick_tsdf + row);
        const Quad t1 = *reinterpret_cast<const Quad*>(brick_tsdf + row + 4);
        const Quad w0 = *reinterpret_cast<const Quad*>(brick_weight + row);
        const Quad w1 = *reinterpret_cast<const Quad*>(brick_weight + row + 4);
        if (take == 0xffu) {  // all 8 voxels: they are inside the window, so the row is whole
            *reinterpret_cast<Quad*>(tsdf + r.at) = t0;
            *reinterpret_cast<Quad*>(tsdf + r.at + 4) = t1;
            *reinterpret_cast<Quad*>(weight + r.at) = w0;
            *reinterpret_cast<Quad*>(weight + r.at + 4) = w1;
        } else {
#pragma unroll
            for (int j = 0; j < kBrick; ++j)
                if (take >> j & 1u) {
                    tsdf[r.at + j] = j < 4 ? t0.v[j & 3] : t1.v[j & 3];
                    weight[r.at + j] = j < 4 ? w0.v[j & 3] : w1.v[j & 3];
                }
        }
        if (COLOUR) {
            uint4 c[kBrick];
#pragma unroll
            for (int j = 0; j < kBrick; ++j)
                if (take >> j & 1u) c[j] = brick_colour[row + j];
#pragma unroll
            for (int j = 0; j < kBrick; ++j)
                if (take >> j & 1u) colour[r.at + j] = c[j];
        }
    }
}

int clamp_shift(int s, int n) { return s < -n ? -n : (s > n ? n : s); }

// leaving: the retained ranges are those of the source voxels lsf_volume_shift keeps (u - s inside), else those of the
// destination voxels it fills (v + s inside)
int convert(const lsf_volume_bricks_params* q, BricksDev& p, bool leaving) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->depth < 1 || q->height < 1 || q->width < 1) return LSF_ERR_BAD_ARGUMENT;
    if ((long long)q->depth * q->height * q->width > 0x7fffffffll) return LSF_ERR_BAD_DIMS;
    const int n[3] = {q->width, q->height, q->depth};
    const int g[3] = {q->origin_x, q->origin_y, q->origin_z};
    const int s[3] = {q->shift_x, q->shift_y, q->shift_z};
    int lo[3], hi[3], b0[3], nb[3];
    long long bricks = 1;
    for (int j = 0; j < 3; ++j) {
        const long long mag = g[j] < 0 ? -(long long)g[j] : (long long)g[j];
        if (mag + n[j] > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
        const int c = leaving ? -clamp_shift(s[j], n[j]) : clamp_shift(s[j], n[j]);
        lo[j] = c < 0 ? -c : 0;
        hi[j] = c > 0 ? n[j] - c : n[j];
        b0[j] = floor_div8(g[j]);
        nb[j] = floor_div8(g[j] + n[j] - 1) - b0[j] + 1;
        bricks *= nb[j];
    }
    if (bricks > 0x7fffffffll) return LSF_ERR_BAD_DIMS;
    p.nx = n[0]; p.ny = n[1]; p.nz = n[2];
    p.gx = g[0]; p.gy = g[1]; p.gz = g[2];
    p.lo_x = lo[0]; p.hi_x = hi[0]; p.lo_y = lo[1]; p.hi_y = hi[1]; p.lo_z = lo[2]; p.hi_z = hi[2];
    p.bx0 = b0[0]; p.by0 = b0[1]; p.bz0 = b0[2];
    p.nbx = nb[0]; p.nby = nb[1]; p.nbz = nb[2];
    p.nbricks = (int)bricks;
    return 0;
}

int blocks_for(long long bricks) {
    const long long want = (bricks + kBricksPerBlock - 1) / kBricksPerBlock;
    return want > kMaxBlocks ? kMaxBlocks : (int)want;
}

struct Span {
    const void* at;
    size_t bytes;
};

// no output overlaps an input or another output
template <int NI, int NO>
bool any_alias(const Span (&ins)[NI], const Span (&outs)[NO]) {
    for (int i = 0; i < NO; ++i) {
        for (int j = 0; j < NI; ++j)
            if (overlaps(outs[i].at, outs[i].bytes, ins[j].at, ins[j].bytes)) return true;
        for (int j = i + 1; j < NO; ++j)
            if (overlaps(outs[i].at, outs[i].bytes, outs[j].at, outs[j].bytes)) return true;
    }
    return false;
}

bool misaligned(uintptr_t bits, uintptr_t mask) { return (bits & mask) != 0; }

}  // namespace

extern "C" int lsf_volume_bricks_count(const float* weight, int32_t* flags, int32_t* offsets, int64_t* total,
                                       const lsf_volume_bricks_params* params, void* stream) {
    (void)hipGetLastError();
    BricksDev p;
    if (int e = convert(params, p, true)) return e;
    if (!weight || !flags || !offsets || !total) return LSF_ERR_BAD_ARGUMENT;
    if (misaligned((uintptr_t)weight | (uintptr_t)flags | (uintptr_t)offsets, 3) || misaligned((uintptr_t)total, 7))
        return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.nx * p.ny * p.nz, nb = (size_t)p.nbricks;
    const Span ins[1] = {{weight, n * 4}};
    const Span outs[3] = {{flags, nb * 4}, {offsets, nb * 4}, {total, 8}};
    if (any_alias(ins, outs)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(bricks_flag_kernel, dim3(blocks_for(p.nbricks)), dim3(kBlock), 0, s,
                       reinterpret_cast<const unsigned*>(weight), flags, p);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(bricks_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, flags, offsets,
                       reinterpret_cast<long long*>(total), p.nbricks);
    return launch_status();
}

extern "C" int lsf_volume_bricks_gather(const float* tsdf, const float* weight, const float* colour,
                                        const int32_t* flags, const int32_t* offsets, int64_t brick_count,
                                        int32_t* out_coords, float* out_tsdf, float* out_weight, float* out_colour,
                                        uint8_t* out_valid, const lsf_volume_bricks_params* params, void* stream) {
    (void)hipGetLastError();
    BricksDev p;
    if (int e = convert(params, p, true)) return e;
    if (!tsdf || !weight || !flags || !offsets || !out_coords || !out_tsdf || !out_weight || !out_valid)
        return LSF_ERR_BAD_ARGUMENT;
    if ((colour == nullptr) != (out_colour == nullptr)) return LSF_ERR_BAD_ARGUMENT;
    if (brick_count < 0 || brick_count > p.nbricks) return LSF_ERR_BAD_ARGUMENT;
    const uintptr_t words = (uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)flags | (uintptr_t)offsets |
                            (uintptr_t)out_coords | (uintptr_t)out_tsdf | (uintptr_t)out_weight;
    if (misaligned(words, 3) || misaligned((uintptr_t)colour | (uintptr_t)out_colour, 15)) return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.nx * p.ny * p.nz, nb = (size_t)p.nbricks, k = (size_t)brick_count;
    const Span ins[5] = {{tsdf, n * 4}, {weight, n * 4}, {colour, n * 16}, {flags, nb * 4}, {offsets, nb * 4}};
    const Span outs[5] = {{out_coords, k * 12}, {out_tsdf, k * kBrickVoxels * 4}, {out_weight, k * kBrickVoxels * 4},
                          {out_colour, k * kBrickVoxels * 16}, {out_valid, k * kWave}};
    if (any_alias(ins, outs)) return LSF_ERR_BAD_ARGUMENT;
    if (brick_count == 0) return 0;
    hipStream_t s = as_stream(stream);
    const unsigned* t = reinterpret_cast<const unsigned*>(tsdf);
    const unsigned* w = reinterpret_cast<const unsigned*>(weight);
    unsigned* ot = reinterpret_cast<unsigned*>(out_tsdf);
    unsigned* ow = reinterpret_cast<unsigned*>(out_weight);
    const dim3 grid(blocks_for(p.nbricks));
    if (colour)
        hipLaunchKernelGGL(bricks_gather_kernel<true>, grid, dim3(kBlock), 0, s, t, w,
                           reinterpret_cast<const uint4*>(colour), flags, offsets, (long long)brick_count, out_coords, ot,
                           ow, reinterpret_cast<uint4*>(out_colour), out_valid, p);
    else
        hipLaunchKernelGGL(bricks_gather_kernel<false>, grid, dim3(kBlock), 0, s, t, w, (const uint4*)nullptr, flags,
                           offsets, (long long)brick_count, out_coords, ot, ow, (uint4*)nullptr, out_valid, p);
    return launch_status();
}

extern "C" int lsf_volume_bricks_scatter(const int32_t* coords, const float* brick_tsdf, const float* brick_weight,
                                         const float* brick_colour, const uint8_t* brick_valid, int64_t brick_count,
                                         float* tsdf, float* weight, float* colour,
                                         const lsf_volume_bricks_params* params, void* stream) {
    (void)hipGetLastError();
    BricksDev p;
    if (int e = convert(params, p, false)) return e;
    if (!coords || !brick_tsdf || !brick_weight || !brick_valid || !tsdf || !weight) return LSF_ERR_BAD_ARGUMENT;
    if ((brick_colour == nullptr) != (colour == nullptr)) return LSF_ERR_BAD_ARGUMENT;
    if (brick_count < 0 || brick_count > 0x7fffffffll) return LSF_ERR_BAD_ARGUMENT;
    const uintptr_t words = (uintptr_t)coords | (uintptr_t)brick_tsdf | (uintptr_t)brick_weight | (uintptr_t)tsdf |
                            (uintptr_t)weight;
    if (misaligned(words, 3) || misaligned((uintptr_t)brick_colour | (uintptr_t)colour, 15)) return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.nx * p.ny * p.nz, k = (size_t)brick_count;
    const Span ins[5] = {{coords, k * 12}, {brick_tsdf, k * kBrickVoxels * 4}, {brick_weight, k * kBrickVoxels * 4},
                         {brick_colour, k * kBrickVoxels * 16}, {brick_valid, k * kWave}};
    const Span outs[3] = {{tsdf, n * 4}, {weight, n * 4}, {colour, n * 16}};
    if (any_alias(ins, outs)) return LSF_ERR_BAD_ARGUMENT;
    if (brick_count == 0) return 0;
    hipStream_t s = as_stream(stream);
    const unsigned* bt = reinterpret_cast<const unsigned*>(brick_tsdf);
    const unsigned* bw = reinterpret_cast<const unsigned*>(brick_weight);
    unsigned* t = reinterpret_cast<unsigned*>(tsdf);
    unsigned* w = reinterpret_cast<unsigned*>(weight);
    const dim3 grid(blocks_for(brick_count));
    if (colour)
        hipLaunchKernelGGL(bricks_scatter_kernel<true>, grid, dim3(kBlock), 0, s, coords, bt, bw,
                           reinterpret_cast<const uint4*>(brick_colour), brick_valid, (long long)brick_count, t, w,
                           reinterpret_cast<uint4*>(colour), p);
    else
        hipLaunchKernelGGL(bricks_scatter_kernel<false>, grid, dim3(kBlock), 0, s, coords, bt, bw, (const uint4*)nullptr,
                           brick_valid, (long long)brick_count, t, w, (uint4*)nullptr, p);
    return launch_status();
}
