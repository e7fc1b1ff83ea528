// The Euclidean distance field of the canonical model (include/lsf_hip.h, lsf_esdf_compute; INTEGRATION.md section 3,
// "Euclidean distance field"; tests/esdf_restatement.py restates it): for every voxel the key
//     min over the sites s of (|v - s|^2, flat(s)),  lexicographic,
// capped at R^2, from which distance2, nearest and the signed metric esdf follow.  A site is an observed voxel with an
// observed 6-neighbour on the other side of iso (and, with unknown = occupied, every voxel that is not observed).
// The key is separable, and flat order is the lexicographic order of (z, y, x), so three partial minima compose to it,
// ties included:
//   x pass   per voxel the nearest site of its own row within R, the smaller x' on a tie: the signed offset dx
//   y pass   min over |dy| <= R of (dx(y + dy)^2 + dy^2, dy, dx(y + dy)): the offsets (dy, dx) within the plane, packed
//   z pass   min over |dz| <= R of (dx^2 + dy^2 + dz^2, flat) over the plane offsets at z + dz: the outputs
// Only integers until the last line of the z pass.  Storing offsets instead of distances and indices keeps every
// intermediate one int32 per voxel: the two scratch volumes.
// The x pass also finds the sites, so no flag volume exists: a wave owns a row (z, y) and sweeps it twice in chunks of 64
// voxels.  Forward, a lane classifies its voxel from tsdf and weight of the voxel and its six neighbours, the wave's
// ballot is the chunk's site mask, the nearest site at or below a lane is the highest mask bit at or below it, or the
// last site of the chunks before (one wave-uniform integer), and the lane stores that distance.  Backward, a lane reads
// its own store back (a stored 0 is the site flag), the ballot is the same mask, the nearest site at or above is the
// lowest bit at or above, or the first site of the chunks after, and the lane stores the nearer of the two, the lower on a
// tie.  Rows of any width take the same path; the work per voxel does not grow with R.
// The y and z passes are windowed scans, exact and bounded: lanes along x (a wave-instruction reads 256 contiguous bytes
// of the row at y + dy or of the plane at z + dz), the walk along the strided axis outwards from the voxel, k = 0, 1,
// ..., min(R, the distance to the farther face), and it ends early once k^2 exceeds the best distance so far, since
// every later candidate is farther and cannot tie.  Near a surface that is a few steps; in free space beyond R it is the
// whole window, which is what bounds the two passes (profiles/esdf_cost.md).  The rows a walk reads are the rows its
// neighbours in y or z read one step earlier or later, so they come from the vector L1 and the L2, not from HBM.
// Grids are capped (LSF_ESDF_MAX_BLOCKS workgroups, eight per CU) with a stride loop behind them, so the record costs
// one atomic per wave (sites) or two per workgroup (finite, max_distance2) whatever the volume's size.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kMaxBlocks = LSF_ESDF_MAX_BLOCKS;
constexpr int kRowsPerBlock = kBlock / kWave;
static_assert(kRowsPerBlock == LSF_ESDF_BLOCK_ROWS, "a wave per row");
static_assert(kBlock == LSF_ESDF_BLOCK_VOXELS, "a voxel per lane");
constexpr int kFar = LSF_ESDF_FAR;
constexpr int kNoSite = 0x7fffffff;  // x pass: no site of the row within R; a real offset is at most 4096 in size
constexpr int kNoPair = -1;          // y pass: no site of the plane within R; a packed pair is never negative
constexpr int kBias = LSF_ESDF_MAX_DISTANCE;  // offsets -4096 .. 4096 stored as 0 .. 8192: 14 bits
constexpr int kPairShift = 14;
static_assert(2 * kBias < (1 << kPairShift), "an offset fits its field");

struct EsdfDev {
    int nx, ny, nz;
    int radius, radius2;
    int occupied;
    float iso, min_weight, voxel_size;
    long long rows;   // nz * ny
    long long plane;  // ny * nx
    long long n;      // nz * ny * nx <= 2^31 - 1
};

// 0: not observed; 1: observed, not inside; 2: inside.  NaN weight is not observed, NaN tsdf is not inside.
__device__ inline int voxel_class(float t, float w, const EsdfDev& p) {
    return w > p.min_weight ? (t < p.iso ? 2 : 1) : 0;
}

// lexicographic (dy, dx) order is the integer order of the packed pair
__device__ inline int pack_pair(int dy, int dx) { return ((dy + kBias) << kPairShift) | (dx + kBias); }

__global__ __launch_bounds__(kBlock) void esdf_x_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         int* __restrict__ offset_x, unsigned long long* record,
                                                         EsdfDev p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const long long stride = (long long)gridDim.x * kRowsPerBlock;
    const int chunks = (p.nx + kWave - 1) / kWave;
    unsigned long long sites = 0;  // wave-uniform
    for (long long row = (long long)blockIdx.x * kRowsPerBlock + wave; row < p.rows; row += stride) {
        const int z = (int)(row / p.ny), y = (int)(row - (long long)z * p.ny);
        const long long at = row * p.nx;
        int last = -1;  // the last site of the chunks before this one
        for (int c = 0; c < chunks; ++c) {
            const int x = c * kWave + lane;
            bool site = false;
            if (x < p.nx) {
                const long long v = at + x;
                const int own = voxel_class(tsdf[v], weight[v], p);
                if (own == 0) {
                    site = p.occupied != 0;
                } else {
                    const int other = 3 - own;
                    if (x > 0) site |= voxel_class(tsdf[v - 1], weight[v - 1], p) == other;
                    if (x + 1 < p.nx) site |= voxel_class(tsdf[v + 1], weight[v + 1], p) == other;
                    if (y > 0) site |= voxel_class(tsdf[v - p.nx], weight[v - p.nx], p) == other;
                    if (y + 1 < p.ny) site |= voxel_class(tsdf[v + p.nx], weight[v + p.nx], p) == other;
                    if (z > 0) site |= voxel_class(tsdf[v - p.plane], weight[v - p.plane], p) == other;
                    if (z + 1 < p.nz) site |= voxel_class(tsdf[v + p.plane], weight[v + p.plane], p) == other;
                }
            }
            const unsigned long long mask = __ballot(site);
            sites += (unsigned long long)__popcll(mask);
            const unsigned long long below = mask & (~0ull >> (kWave - 1 - lane));  // the sites at or below this lane
            const int left = below ? c * kWave + (kWave - 1 - __clzll((long long)below)) : last;
            if (x < p.nx) offset_x[at + x] = left >= 0 ? x - left : kNoSite;
            if (mask) last = c * kWave + (kWave - 1 - __clzll((long long)mask));
        }
        int next = -1;  // the first site of the chunks after this one
        for (int c = chunks - 1; c >= 0; --c) {
            const int x = c * kWave + lane;
            int down = kNoSite;
            if (x < p.nx) down = offset_x[at + x];  // this lane's own store of the forward sweep
            const unsigned long long mask = __ballot(down == 0);
            const unsigned long long above = mask >> lane;  // the sites at or above this lane
            const int right = above ? x + (__ffsll((long long)above) - 1) : next;
            const int up = right >= 0 ? right - x : kNoSite;
            // the nearer; the lower x' on a tie; nothing beyond R
            const int out = down <= up ? (down <= p.radius ? -down : kNoSite) : (up <= p.radius ? up : kNoSite);
            if (x < p.nx) offset_x[at + x] = out;
            if (mask) next = c * kWave + (__ffsll((long long)mask) - 1);
        }
    }
    if (lane == 0 && sites) atomicAdd(record, sites);
}

// the farthest step of a walk along an axis of n voxels from position i: R, or the distance to the farther face
__device__ inline int walk_length(int i, int n, int radius) {
    const int reach = i > n - 1 - i ? i : n - 1 - i;
    return reach < radius ? reach : radius;
}

__global__ __launch_bounds__(kBlock) void esdf_y_kernel(const int* __restrict__ offset_x, int* __restrict__ pair_yx,
                                                         EsdfDev p) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < p.n; v += stride) {
        const long long row = v / p.nx;
        const int y = (int)(row % p.ny);
        const int steps = walk_length(y, p.ny, p.radius);
        int best = kFar, best_pair = kNoPair;
        for (int k = 0; k <= steps; ++k) {
            if (k * k > best) break;  // every later candidate is farther
            if (y - k >= 0) {
                const int dx = offset_x[v - (long long)k * p.nx];
                if (dx != kNoSite) {  // else |dx| <= R
                    const int d = dx * dx + k * k;
                    const int pair = pack_pair(-k, dx);
                    if (d <= p.radius2 && (d < best || (d == best && pair < best_pair))) {
                        best = d;
                        best_pair = pair;
                    }
                }
            }
            if (k > 0 && y + k < p.ny) {
                const int dx = offset_x[v + (long long)k * p.nx];
                if (dx != kNoSite) {  // else |dx| <= R
                    const int d = dx * dx + k * k;
                    const int pair = pack_pair(k, dx);
                    if (d <= p.radius2 && (d < best || (d == best && pair < best_pair))) {
                        best = d;
                        best_pair = pair;
                    }
                }
            }
        }
        pair_yx[v] = best_pair;
    }
}

__global__ __launch_bounds__(kBlock) void esdf_z_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         const int* __restrict__ pair_yx, int* __restrict__ distance2,
                                                         int* __restrict__ nearest, float* __restrict__ esdf,
                                                         unsigned long long* record, EsdfDev p) {
    __shared__ int wave_finite[kBlock / kWave], wave_max[kBlock / kWave];
    const long long stride = (long long)gridDim.x * kBlock;
    int finite = 0, largest = 0;
    for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < p.n; v += stride) {
        const int z = (int)(v / p.plane);
        const int steps = walk_length(z, p.nz, p.radius);
        int best = kFar, best_flat = -1;
        for (int k = 0; k <= steps; ++k) {
            if (k * k > best) break;
            if (z - k >= 0) {
                const long long at = v - (long long)k * p.plane;
                const int pair = pair_yx[at];
                if (pair != kNoPair) {
                    const int dy = (pair >> kPairShift) - kBias, dx = (pair & ((1 << kPairShift) - 1)) - kBias;
                    const int d = dx * dx + dy * dy + k * k;
                    const int flat = (int)(at + (long long)dy * p.nx + dx);  // the site's own index: inside the volume
                    if (d <= p.radius2 && (d < best || (d == best && flat < best_flat))) {
                        best = d;
                        best_flat = flat;
                    }
                }
            }
            if (k > 0 && z + k < p.nz) {
                const long long at = v + (long long)k * p.plane;
                const int pair = pair_yx[at];
                if (pair != kNoPair) {
                    const int dy = (pair >> kPairShift) - kBias, dx = (pair & ((1 << kPairShift) - 1)) - kBias;
                    const int d = dx * dx + dy * dy + k * k;
                    const int flat = (int)(at + (long long)dy * p.nx + dx);  // the site's own index: inside the volume
                    if (d <= p.radius2 && (d < best || (d == best && flat < best_flat))) {
                        best = d;
                        best_flat = flat;
                    }
                }
            }
        }
        const bool far = best == kFar;
        const float root = far ? (float)p.radius : sqrtf((float)best);
        const float metres = root * p.voxel_size;
        distance2[v] = best;
        nearest[v] = best_flat;
        esdf[v] = voxel_class(tsdf[v], weight[v], p) == 2 ? -metres : metres;
        if (!far) {
            ++finite;
            largest = best > largest ? best : largest;
        }
    }
    // the record: lanes, then the workgroup's waves, then two atomics
#pragma unroll
    for (int step = kWave / 2; step > 0; step >>= 1) {
        finite += __shfl_down(finite, step);
        const int other = __shfl_down(largest, step);
        largest = other > largest ? other : largest;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
        wave_finite[wave] = finite;
        wave_max[wave] = largest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0, most = 0;
        for (int w = 0; w < kBlock / kWave; ++w) {
            total += (unsigned long long)wave_finite[w];
            most = (unsigned long long)wave_max[w] > most ? (unsigned long long)wave_max[w] : most;
        }
        if (total) {
            atomicAdd(record + 1, total);
            atomicMax(record + 2, most);
        }
    }
}

int convert(const lsf_esdf_params* q, EsdfDev& p) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->depth < 1 || q->height < 1 || q->width < 1) return LSF_ERR_BAD_ARGUMENT;
    if (q->max_distance_voxels < 1 || q->max_distance_voxels > LSF_ESDF_MAX_DISTANCE) return LSF_ERR_BAD_ARGUMENT;
    if (!(q->voxel_size > 0.0) || !(q->voxel_size <= 1.7976931348623157e308)) return LSF_ERR_BAD_ARGUMENT;  // NaN too
    if (q->iso != q->iso || q->min_weight != q->min_weight) return LSF_ERR_BAD_ARGUMENT;
    if (q->unknown != LSF_ESDF_UNKNOWN_FREE && q->unknown != LSF_ESDF_UNKNOWN_OCCUPIED) return LSF_ERR_BAD_ARGUMENT;
    if (q->passes < 1 || q->passes > LSF_ESDF_PASSES_ALL) return LSF_ERR_BAD_ARGUMENT;
    p.rows = (long long)q->depth * q->height;
    p.plane = (long long)q->height * q->width;
    if (p.rows > 0x7fffffffll || p.rows * q->width > 0x7fffffffll) return LSF_ERR_BAD_DIMS;
    p.n = p.rows * q->width;
    p.nx = q->width; p.ny = q->height; p.nz = q->depth;
    p.radius = q->max_distance_voxels;
    p.radius2 = p.radius * p.radius;
    p.occupied = q->unknown == LSF_ESDF_UNKNOWN_OCCUPIED;
    p.iso = q->iso;
    p.min_weight = q->min_weight;
    p.voxel_size = (float)q->voxel_size;
    return 0;
}

int capped(long long want) { return want > kMaxBlocks ? kMaxBlocks : (int)want; }

}  // namespace

extern "C" int lsf_esdf_compute(const float* tsdf, const float* weight, int32_t* scratch_a, int32_t* scratch_b,
                                int32_t* distance2, int32_t* nearest, float* esdf, int64_t* record,
                                const lsf_esdf_params* params, void* stream) {
    (void)hipGetLastError();
    EsdfDev p;
    if (int e = convert(params, p)) return e;
    const void* const buffers[8] = {tsdf, weight, scratch_a, scratch_b, distance2, nearest, esdf, record};
    const size_t volume = (size_t)p.n * 4;
    const size_t bytes[8] = {volume, volume, volume, volume, volume, volume, volume, LSF_ESDF_RECORD_WORDS * 8};
    for (int i = 0; i < 8; ++i) {
        if (!buffers[i] || ((uintptr_t)buffers[i] & (i == 7 ? 7 : 3)) != 0) return LSF_ERR_BAD_ARGUMENT;
        for (int j = i < 2 ? 2 : i + 1; j < 8; ++j)  // the two inputs may be one buffer; nothing else may share memory
            if (overlaps(buffers[i], bytes[i], buffers[j], bytes[j])) return LSF_ERR_BAD_ARGUMENT;
    }
    hipStream_t s = as_stream(stream);
    unsigned long long* r = reinterpret_cast<unsigned long long*>(record);
    if (hipError_t e = hipMemsetAsync(record, 0, LSF_ESDF_RECORD_WORDS * 8, s)) return (int)e;
    if (params->passes & LSF_ESDF_PASS_X)
        hipLaunchKernelGGL(esdf_x_kernel, dim3(capped((p.rows + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(kBlock), 0, s,
                           tsdf, weight, scratch_b, r, p);
    const int blocks = capped((p.n + kBlock - 1) / kBlock);
    if (params->passes & LSF_ESDF_PASS_Y)
        hipLaunchKernelGGL(esdf_y_kernel, dim3(blocks), dim3(kBlock), 0, s, scratch_b, scratch_a, p);
    if (params->passes & LSF_ESDF_PASS_Z)
        hipLaunchKernelGGL(esdf_z_kernel, dim3(blocks), dim3(kBlock), 0, s, tsdf, weight, scratch_a, distance2, nearest,
                           esdf, r, p);
    return launch_status();
}
