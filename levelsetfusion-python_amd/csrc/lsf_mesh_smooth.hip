// Taubin smoothing of a triangle mesh and vertex normals rebuilt from its faces (include/lsf_hip.h,
// lsf_mesh_smooth_prepare / _run, lsf_mesh_vertex_normals).  The contract is INTEGRATION.md section 3 ("Mesh smoothing");
// tests/mesh_smooth_restatement.py restates it and the kernels equal it bit for bit.
// Edges: every face contributes its corner pairs (0,1), (1,2), (2,0); a pair with equal ends is skipped, every other pair
// adds 1 to the face count of the undirected edge {a, b}.  N(i): the distinct vertices an edge joins to i; d(i) its size.
// Pinned (boundary_fixed): the ends of every edge whose face count is not 2.  A pinned vertex and one with d = 0 stay.
// One pass with weight w: B = the largest |coordinate| of the input, an integer maximum on the float bits; E = the
// exponent field of B's bits; e = max(E, 1) - 126; q = 2^(e-32), 1 when B = 0; Q(x) = (int64) rint(double(x) / q), 0 for a
// non-finite x; S_i = sum of Q(p_j) over N(i), in integers; m = (double(S_i) * q) / double(d(i));
// p_i' = float32(double(p_i) + w * (m - double(p_i))), every operation rounded on its own (-ffp-contract=off).
// q and 1 / q are powers of two between 2^-157 and 2^157 and |x| / q is 0 or within [2^-246, 2^32): the kernel multiplies
// by 1 / q, which gives the bits of the division.  The sums are integers, so the order in which a row's cursors were
// handed out, the launch shape and the table's size change no bit; the maxima are integer maxima.
// Normals: c = (p_b - p_a) x (p_c - p_a) in float64; M = the largest |component| by an integer maximum on the doubles'
// bits; em = max(E, 1) - 1022 with E the exponent field of M's bits; qn = 2^(em-32), 1 when M = 0; every face adds
// (int64) rint(c / qn), 0 for a non-finite component, to its three vertices by 64-bit integer atomics; the normal is
// float32(S / sqrt((S_x^2 + S_y^2) + S_z^2)), and (0, 0, 0) when the length is 0.
// The edges live in an open-addressing table of 64-bit keys (lo << 32) | hi claimed by compare-and-swap; a probe walk ends
// after `slots` steps (table_overflow).  Degrees are counted when a key is claimed, scanned into row offsets by tile counts
// and one scan workgroup, and the compressed-row neighbour list is filled from the table through per-vertex cursors.
// Loops: probes <= slots; a row's gather takes d(i) <= 2E steps and never reads past the list's 6F words.
// No float atomics, no inter-workgroup waits.  Every launch but the one-workgroup scan walks tiles of
// LSF_MESH_SMOOTH_TILE = 256 consecutive items, one per lane, on a grid capped at params.max_blocks (at most
// LSF_MESH_SMOOTH_MAX_BLOCKS) workgroups with a stride loop behind it.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kTile = LSF_MESH_SMOOTH_TILE;
constexpr int kScanThreads = LSF_MESH_SMOOTH_SCAN_THREADS;
constexpr int kWaves = kBlock / kWave;
constexpr unsigned long long kEmpty = ~0ull;
static_assert(kTile == kBlock, "one item per lane");

enum Field {
    kVerticesIn, kFacesIn, kInvalidVertices, kInvalidFaces, kEdges, kBoundaryEdges, kNonmanifoldEdges, kPinnedVertices,
    kIsolatedVertices, kMaxDegree, kTableOverflow, kNonfiniteOut, kZeroNormals
};
static_assert(kZeroNormals + 1 == LSF_MESH_SMOOTH_RECORD_WORDS, "the record's fields");

// scalars: B's bits of the input, the passes' three rotating maxima, M's bits
enum Scalar { kInputMax, kRotating, kNormalMax = kRotating + 3 };
static_assert(kNormalMax + 1 == LSF_MESH_SMOOTH_SCALAR_WORDS, "the scalar words");

struct Dev {
    int V, F;
    int tiles_v, tiles_f, tiles_s;
    unsigned slots, mask;
    long long list_words;  // max(6F, 1): the neighbour list's size
    int fixed;
    const float* __restrict__ vertices;
    const int* __restrict__ faces;
    int *degree, *pinned, *row, *cursor;  // planes of vertex_work
    unsigned long long* keys;
    int* counts;
    int* offsets;
    int* neighbours;
    unsigned long long* scalars;
    unsigned long long* record;
};
static_assert(LSF_MESH_SMOOTH_VERTEX_WORDS == 4, "degree, pinned, row offset, cursor");

__device__ inline unsigned hash2(unsigned a, unsigned b) {
    unsigned h = a * 0x9E3779B1u;
    h = (h ^ (h >> 15)) + b * 0x85EBCA77u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    return h ^ (h >> 16);
}

__device__ inline unsigned block_sum(unsigned value) {
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int d = kWave / 2; d > 0; d /= 2) value += __shfl_xor(value, d, kWave);
    __syncthreads();  // the words of the call before are read
    if (lane == 0) sh[wave] = value;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += sh[w];
    return total;
}

// the sum of `value` over the lanes below this one; every lane of the workgroup calls it
__device__ inline unsigned block_prefix(unsigned value) {
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned incl = value;
#pragma unroll
    for (int s = 1; s < kWave; s *= 2) {
        const unsigned y = __shfl_up(incl, s, kWave);
        if (lane >= s) incl += y;
    }
    __syncthreads();  // the words of the call before are read
    if (lane == kWave - 1) sh[wave] = incl;
    __syncthreads();
    unsigned prefix = incl - value;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) prefix += w < wave ? sh[w] : 0u;
    return prefix;
}

// 2^e as a double, e in -1022 .. 1023
__device__ inline double pow2(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }

__device__ inline void add_to_record(const Dev& d, int field, unsigned value) {
    const unsigned total = block_sum(value);
    if (threadIdx.x == 0 && total) atomicAdd(d.record + field, (unsigned long long)total);
}

__global__ void begin_kernel(Dev d) {
    if (threadIdx.x < LSF_MESH_SMOOTH_RECORD_WORDS)
        d.record[threadIdx.x] = threadIdx.x == kVerticesIn ? (unsigned long long)d.V
                                : threadIdx.x == kFacesIn  ? (unsigned long long)d.F
                                                           : 0ull;
    if (threadIdx.x < LSF_MESH_SMOOTH_SCALAR_WORDS) d.scalars[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kBlock) void init_kernel(Dev d) {
    unsigned bad = 0, top = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p = d.vertices[i * 3 + a];
            ok = ok && isfinite(p);
            top = max(top, __float_as_uint(p) & 0x7fffffffu);
        }
        d.degree[i] = 0;
        d.pinned[i] = 0;
        bad += ok ? 0u : 1u;
    }
    const unsigned long long m = wave_max_u64((unsigned long long)top);
    if (threadIdx.x % kWave == 0 && m) atomicMax(d.scalars + kInputMax, m);
    add_to_record(d, kInvalidVertices, bad);
}

// the slot of the key: claimed, or met holding it.  At most `slots` probes; -1 when the table is full.
__device__ inline long long claim(const Dev& d, unsigned long long key, bool& claimed) {
    unsigned h = hash2((unsigned)(key >> 32), (unsigned)key) & d.mask;
    claimed = false;
    for (unsigned n = 0; n < d.slots; ++n) {
        const unsigned long long cur = atomicCAS(&d.keys[h], kEmpty, key);
        if (cur == kEmpty) {
            claimed = true;
            return h;
        }
        if (cur == key) return h;
        h = (h + 1u) & d.mask;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void insert_kernel(Dev d) {
    unsigned bad = 0, lost = 0;
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        if (f >= d.F) continue;
        const int v[3] = {d.faces[f * 3], d.faces[f * 3 + 1], d.faces[f * 3 + 2]};
        if ((unsigned)v[0] >= (unsigned)d.V || (unsigned)v[1] >= (unsigned)d.V || (unsigned)v[2] >= (unsigned)d.V) {
            ++bad;  // before any gather
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int a = v[k], b = v[(k + 1) % 3];
            if (a == b) continue;
            const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
            bool claimed;
            const long long slot = claim(d, ((unsigned long long)lo << 32) | hi, claimed);
            if (slot < 0) {
                ++lost;
                continue;
            }
            atomicAdd(&d.counts[slot], 1);
            if (claimed) {
                atomicAdd(&d.degree[lo], 1);
                atomicAdd(&d.degree[hi], 1);
            }
        }
    }
    add_to_record(d, kInvalidFaces, bad);
    add_to_record(d, kTableOverflow, lost);
}

// the ends of the edge a slot holds; false for an empty slot (and for a key no insert wrote)
__device__ inline bool edge_of(const Dev& d, long long slot, int& lo, int& hi) {
    const unsigned long long key = d.keys[slot];
    lo = (int)(key >> 32);
    hi = (int)(unsigned)key;
    return key != kEmpty && (unsigned)lo < (unsigned)d.V && (unsigned)hi < (unsigned)d.V;
}

__global__ __launch_bounds__(kBlock) void edge_kernel(Dev d) {
    unsigned edges = 0, border = 0, shared = 0;
    for (int tile = blockIdx.x; tile < d.tiles_s; tile += gridDim.x) {
        const long long s = (long long)tile * kTile + threadIdx.x;
        int lo, hi;
        if (s >= (long long)d.slots || !edge_of(d, s, lo, hi)) continue;
        const int n = d.counts[s];
        ++edges;
        border += n == 1 ? 1u : 0u;
        shared += n > 2 ? 1u : 0u;
        if (d.fixed && n != 2) {
            d.pinned[lo] = 1;  // (every writer writes 1)
            d.pinned[hi] = 1;
        }
    }
    add_to_record(d, kEdges, edges);
    add_to_record(d, kBoundaryEdges, border);
    add_to_record(d, kNonmanifoldEdges, shared);
}

__global__ __launch_bounds__(kBlock) void degree_kernel(Dev d) {
    unsigned pinned = 0, isolated = 0, most = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const unsigned n = i < d.V ? (unsigned)d.degree[i] : 0u;
        if (i < d.V) {
            pinned += d.pinned[i] ? 1u : 0u;
            isolated += n == 0 ? 1u : 0u;
            most = max(most, n);
        }
        const unsigned total = block_sum(n);
        if (threadIdx.x == 0) d.offsets[tile] = (int)total;
    }
    const unsigned long long m = wave_max_u64((unsigned long long)most);
    if (threadIdx.x % kWave == 0 && m) atomicMax(d.record + kMaxDegree, m);
    add_to_record(d, kPinnedVertices, pinned);
    add_to_record(d, kIsolatedVertices, isolated);
}

// one workgroup: the tile counts become their exclusive prefix, in place (the total is 2E <= 6F, below 2^31).  `tiles` may
// exceed the lane count: the workgroup loops.
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int* __restrict__ a, int tiles) {
    __shared__ long long sh[kScanThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    long long running = 0;
    for (int base = 0; base < tiles; base += kScanThreads) {
        const int idx = base + threadIdx.x;
        const long long x = idx < tiles ? a[idx] : 0;
        long long incl = x;
#pragma unroll
        for (int s = 1; s < kWave; s *= 2) {
            const long long y = __shfl_up(incl, s, kWave);
            if (lane >= s) incl += y;
        }
        if (lane == kWave - 1) sh[wave] = incl;
        __syncthreads();
        long long before = 0, step = 0;
        for (int w = 0; w < kScanThreads / kWave; ++w) {
            before += w < wave ? sh[w] : 0;
            step += sh[w];
        }
        if (idx < tiles) a[idx] = (int)(running + before + incl - x);
        running += step;
        __syncthreads();  // sh is rewritten by the next step
    }
}

__global__ __launch_bounds__(kBlock) void rows_kernel(Dev d) {
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const unsigned n = i < d.V ? (unsigned)d.degree[i] : 0u;
        const unsigned row = (unsigned)d.offsets[tile] + block_prefix(n);
        if (i < d.V) {
            d.row[i] = (int)row;
            d.cursor[i] = (int)row;
        }
    }
}

__global__ __launch_bounds__(kBlock) void fill_kernel(Dev d) {
    for (int tile = blockIdx.x; tile < d.tiles_s; tile += gridDim.x) {
        const long long s = (long long)tile * kTile + threadIdx.x;
        int lo, hi;
        if (s >= (long long)d.slots || !edge_of(d, s, lo, hi)) continue;
        const long long at_lo = atomicAdd(&d.cursor[lo], 1), at_hi = atomicAdd(&d.cursor[hi], 1);
        if (at_lo >= 0 && at_lo < d.list_words) d.neighbours[at_lo] = hi;
        if (at_hi >= 0 && at_hi < d.list_words) d.neighbours[at_hi] = lo;
    }
}

__global__ void run_begin_kernel(Dev d) {
    if (threadIdx.x < 3) d.scalars[kRotating + threadIdx.x] = threadIdx.x == 0 ? d.scalars[kInputMax] : 0ull;
    if (threadIdx.x == 0) d.record[kNonfiniteOut] = 0ull;
}

// pass k reads its B from scalars[kRotating + k % 3], leaves its output's in the next word and zeroes the word after that,
// which the pass before read and the next pass will add to
__global__ __launch_bounds__(kBlock) void pass_kernel(Dev d, const float* __restrict__ src, float* __restrict__ dst,
                                                      double w, int word_in, int word_out, int word_zero, int last) {
    const unsigned b_bits = (unsigned)d.scalars[word_in];
    const int e = max((int)(b_bits >> 23), 1) - 126 - 32;
    const double q = b_bits ? pow2(e) : 1.0, q_inv = b_bits ? pow2(-e) : 1.0;
    unsigned top = 0, bad = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        float p[3], o[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = p[a] = src[i * 3 + a];
        const int n = d.degree[i];
        if (!d.pinned[i] && n > 0) {
            const long long row = d.row[i];
            long long sum[3] = {0, 0, 0};
            for (int j = 0; j < n; ++j) {  // n = d(i) <= 2E
                const long long at = row + j;
                if (at < 0 || at >= d.list_words) break;
                const long long v = d.neighbours[at];
                if ((unsigned long long)v >= (unsigned long long)d.V) continue;  // before the gather
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = src[v * 3 + a];
                    sum[a] += isfinite(x) ? (long long)rint((double)x * q_inv) : 0ll;
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double m = ((double)sum[a] * q) / (double)n;
                o[a] = (float)((double)p[a] + w * (m - (double)p[a]));
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            dst[i * 3 + a] = o[a];
            top = max(top, __float_as_uint(o[a]) & 0x7fffffffu);
            bad += isfinite(o[a]) ? 0u : 1u;
        }
    }
    const unsigned long long m = wave_max_u64((unsigned long long)top);
    if (threadIdx.x % kWave == 0 && m) atomicMax(d.scalars + word_out, m);
    if (blockIdx.x == 0 && threadIdx.x == 0) d.scalars[word_zero] = 0ull;
    if (last) add_to_record(d, kNonfiniteOut, bad);
}

__global__ void normals_begin_kernel(Dev d, int fresh) {
    if (fresh && threadIdx.x < LSF_MESH_SMOOTH_RECORD_WORDS)
        d.record[threadIdx.x] = threadIdx.x == kVerticesIn ? (unsigned long long)d.V
                                : threadIdx.x == kFacesIn  ? (unsigned long long)d.F
                                                           : 0ull;
    if (threadIdx.x == 0) {
        d.record[kZeroNormals] = 0ull;
        d.scalars[kNormalMax] = 0ull;
    }
}

__global__ __launch_bounds__(kBlock) void validate_kernel(Dev d) {
    unsigned bad = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        bad += isfinite(d.vertices[i * 3]) && isfinite(d.vertices[i * 3 + 1]) && isfinite(d.vertices[i * 3 + 2]) ? 0u : 1u;
    }
    add_to_record(d, kInvalidVertices, bad);
}

// the face's corners and c = (p_b - p_a) x (p_c - p_a) in float64; false, before any gather, for an index outside [0, V)
__device__ inline bool face_cross(const Dev& d, long long f, int (&v)[3], double (&c)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = d.faces[f * 3 + k];
    if ((unsigned)v[0] >= (unsigned)d.V || (unsigned)v[1] >= (unsigned)d.V || (unsigned)v[2] >= (unsigned)d.V)
        return false;
    double u[3], w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double pa = (double)d.vertices[(long long)v[0] * 3 + a];
        u[a] = (double)d.vertices[(long long)v[1] * 3 + a] - pa;
        w[a] = (double)d.vertices[(long long)v[2] * 3 + a] - pa;
    }
    c[0] = u[1] * w[2] - u[2] * w[1];
    c[1] = u[2] * w[0] - u[0] * w[2];
    c[2] = u[0] * w[1] - u[1] * w[0];
    return true;
}

__global__ __launch_bounds__(kBlock) void normal_max_kernel(Dev d, int fresh) {
    unsigned long long top = 0;
    unsigned bad = 0;
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        if (f >= d.F) continue;
        int v[3];
        double c[3];
        if (!face_cross(d, f, v, c)) {
            ++bad;
            continue;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(c[a]) & 0x7fffffffffffffffull;
            top = bits > top ? bits : top;
        }
    }
    const unsigned long long m = wave_max_u64(top);
    if (threadIdx.x % kWave == 0 && m) atomicMax(d.scalars + kNormalMax, m);
    if (fresh) add_to_record(d, kInvalidFaces, bad);
}

__global__ __launch_bounds__(kBlock) void normal_scatter_kernel(Dev d, unsigned long long* __restrict__ sums) {
    const unsigned long long m_bits = d.scalars[kNormalMax];
    const double qn = m_bits ? ldexp(1.0, max((int)(m_bits >> 52), 1) - 1022 - 32) : 1.0;
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        if (f >= d.F) continue;
        int v[3];
        double c[3];
        if (!face_cross(d, f, v, c)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const long long t = isfinite(c[a]) ? (long long)rint(c[a] / qn) : 0ll;
            if (t == 0) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(&sums[(long long)v[k] * 3 + a], (unsigned long long)t);
        }
    }
}

__global__ __launch_bounds__(kBlock) void normalise_kernel(Dev d, const long long* __restrict__ sums,
                                                           float* __restrict__ normals) {
    unsigned zero = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        const double s[3] = {(double)sums[i * 3], (double)sums[i * 3 + 1], (double)sums[i * 3 + 2]};
        const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        zero += len == 0.0 ? 1u : 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[i * 3 + a] = len == 0.0 ? 0.0f : (float)(s[a] / len);
    }
    add_to_record(d, kZeroNormals, zero);
}

int tiles_of(long long n) { return (int)((n + kTile - 1) / kTile); }

struct Range {
    const void* p;
    size_t bytes;
    unsigned align;
};

// a buffer of a size that is not 0 must be given, on its alignment; no written buffer overlaps any other
template <int N>
bool ranges_ok(const Range (&r)[N], int first_written) {
    for (int i = 0; i < N; ++i)
        if (r[i].bytes && (!r[i].p || ((uintptr_t)r[i].p & (r[i].align - 1)) != 0)) return false;
    for (int i = first_written; i < N; ++i)
        for (int j = 0; j < i; ++j)
            if (overlaps(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) return false;
    return true;
}

struct Blocks {
    int v, f, s;
};

// the checks every entry point shares
int convert(const lsf_mesh_smooth_params* q, Dev& d, Blocks& blocks) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->vertex_count < 0 || q->vertex_count > LSF_MESH_SMOOTH_MAX_ITEMS || q->face_count < 0 ||
        q->face_count > LSF_MESH_SMOOTH_MAX_ITEMS)
        return LSF_ERR_BAD_ARGUMENT;
    const long long least = 2ll * (q->face_count > 0 ? 3ll * q->face_count : 1ll), slots = q->table_slots;
    if (slots < 2 || slots > LSF_MESH_SMOOTH_MAX_SLOTS || (slots & (slots - 1)) != 0 || slots < least)
        return LSF_ERR_BAD_ARGUMENT;
    if (q->max_blocks < 0 || q->max_blocks > LSF_MESH_SMOOTH_MAX_BLOCKS) return LSF_ERR_BAD_ARGUMENT;
    for (int flag : {q->boundary_fixed, q->fresh_record})
        if (flag != 0 && flag != 1) return LSF_ERR_BAD_ARGUMENT;
    if (q->reserved != 0 || q->iterations < 0 || q->iterations > LSF_MESH_SMOOTH_MAX_ITERATIONS)
        return LSF_ERR_BAD_ARGUMENT;
    if (!(q->lam > 0.0 && q->lam <= 1.0) || !(q->mu <= 0.0 && q->mu >= -1.7976931348623157e308))
        return LSF_ERR_BAD_ARGUMENT;  // (a NaN fails both comparisons)
    d.V = q->vertex_count;
    d.F = q->face_count;
    d.slots = (unsigned)slots;
    d.mask = (unsigned)slots - 1u;
    d.list_words = d.F > 0 ? 6ll * d.F : 1ll;
    d.fixed = q->boundary_fixed;
    d.tiles_v = tiles_of(d.V);
    d.tiles_f = tiles_of(d.F);
    d.tiles_s = tiles_of(slots);
    const int most = q->max_blocks ? q->max_blocks : LSF_MESH_SMOOTH_MAX_BLOCKS;
    blocks.v = d.tiles_v < most ? d.tiles_v : most;
    blocks.f = d.tiles_f < most ? d.tiles_f : most;
    blocks.s = d.tiles_s < most ? d.tiles_s : most;
    return 0;
}

void cut(Dev& d, int32_t* vertex_work) {
    const long long V = d.V;
    d.degree = vertex_work;
    d.pinned = vertex_work + V;
    d.row = vertex_work + 2 * V;
    d.cursor = vertex_work + 3 * V;
}

}  // namespace

#define LSF_SMOOTH_LAUNCH(kernel, blocks, threads, ...)                                     \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);         \
        if (int e = launch_status()) return e;                                              \
    } while (0)

extern "C" int lsf_mesh_smooth_prepare(const float* vertices, const int32_t* faces, int32_t* vertex_work,
                                       int64_t* edge_keys, int32_t* edge_counts, int32_t* tile_offsets,
                                       int32_t* neighbours, int64_t* scalars, int64_t* record,
                                       const lsf_mesh_smooth_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    Blocks b;
    if (int e = convert(params, d, b)) return e;
    const size_t V = (size_t)d.V, F = (size_t)d.F;
    const Range ranges[9] = {{vertices, V * 12, 4},
                             {faces, F * 12, 4},
                             {vertex_work, V * 4 * LSF_MESH_SMOOTH_VERTEX_WORDS, 4},
                             {edge_keys, (size_t)d.slots * 8, 8},
                             {edge_counts, (size_t)d.slots * 4, 4},
                             {tile_offsets, (size_t)d.tiles_v * 4, 4},
                             {neighbours, (size_t)d.list_words * 4, 4},
                             {scalars, 8 * LSF_MESH_SMOOTH_SCALAR_WORDS, 8},
                             {record, 8 * LSF_MESH_SMOOTH_RECORD_WORDS, 8}};
    if (!ranges_ok(ranges, 2)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, vertex_work);
    d.vertices = vertices;
    d.faces = faces;
    d.keys = reinterpret_cast<unsigned long long*>(edge_keys);
    d.counts = edge_counts;
    d.offsets = tile_offsets;
    d.neighbours = neighbours;
    d.scalars = reinterpret_cast<unsigned long long*>(scalars);
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    LSF_SMOOTH_LAUNCH(begin_kernel, 1, kWave, d);
    if (d.V == 0) {  // no vertex: every face is invalid, and nothing else is to do
        if (d.F > 0) LSF_SMOOTH_LAUNCH(insert_kernel, b.f, kBlock, d);
        return 0;
    }
    LSF_SMOOTH_LAUNCH(init_kernel, b.v, kBlock, d);
    if (d.F > 0) {
        if (hipError_t e = hipMemsetAsync(d.keys, 0xff, (size_t)d.slots * 8, s)) return (int)e;
        if (hipError_t e = hipMemsetAsync(d.counts, 0, (size_t)d.slots * 4, s)) return (int)e;
        LSF_SMOOTH_LAUNCH(insert_kernel, b.f, kBlock, d);
        LSF_SMOOTH_LAUNCH(edge_kernel, b.s, kBlock, d);
    }
    LSF_SMOOTH_LAUNCH(degree_kernel, b.v, kBlock, d);
    LSF_SMOOTH_LAUNCH(scan_kernel, 1, kScanThreads, d.offsets, d.tiles_v);
    LSF_SMOOTH_LAUNCH(rows_kernel, b.v, kBlock, d);
    if (d.F > 0) LSF_SMOOTH_LAUNCH(fill_kernel, b.s, kBlock, d);
    return 0;
}

extern "C" int lsf_mesh_smooth_run(const float* vertices, const int32_t* vertex_work, const int32_t* neighbours,
                                   float* out_vertices, float* scratch, int64_t* scalars, int64_t* record,
                                   const lsf_mesh_smooth_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    Blocks b;
    if (int e = convert(params, d, b)) return e;
    const size_t V = (size_t)d.V;
    const Range ranges[7] = {{vertices, V * 12, 4},
                             {vertex_work, V * 4 * LSF_MESH_SMOOTH_VERTEX_WORDS, 4},
                             {neighbours, (size_t)d.list_words * 4, 4},
                             {out_vertices, V * 12, 4},
                             {scratch, V * 12, 4},
                             {scalars, 8 * LSF_MESH_SMOOTH_SCALAR_WORDS, 8},
                             {record, 8 * LSF_MESH_SMOOTH_RECORD_WORDS, 8}};
    if (!ranges_ok(ranges, 3)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, const_cast<int32_t*>(vertex_work));
    d.vertices = vertices;
    d.faces = nullptr;
    d.keys = nullptr;
    d.counts = nullptr;
    d.offsets = nullptr;
    d.neighbours = const_cast<int32_t*>(neighbours);
    d.scalars = reinterpret_cast<unsigned long long*>(scalars);
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    LSF_SMOOTH_LAUNCH(run_begin_kernel, 1, kWave, d);
    if (d.V == 0) return 0;
    const int per_iteration = params->mu != 0.0 ? 2 : 1, passes = params->iterations * per_iteration;
    if (passes == 0) return (int)hipMemcpyAsync(out_vertices, vertices, V * 12, hipMemcpyDeviceToDevice, s);
    const float* src = vertices;
    for (int k = 0; k < passes; ++k) {
        float* dst = (passes - 1 - k) % 2 == 0 ? out_vertices : scratch;  // the last pass writes out_vertices
        const double w = k % per_iteration == 0 ? params->lam : params->mu;
        LSF_SMOOTH_LAUNCH(pass_kernel, b.v, kBlock, d, src, dst, w, kRotating + k % 3, kRotating + (k + 1) % 3,
                          kRotating + (k + 2) % 3, k == passes - 1 ? 1 : 0);
        src = dst;
    }
    return 0;
}

extern "C" int lsf_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t* sums, float* normals,
                                       int64_t* scalars, int64_t* record, const lsf_mesh_smooth_params* params,
                                       void* stream) {
    (void)hipGetLastError();
    Dev d;
    Blocks b;
    if (int e = convert(params, d, b)) return e;
    const size_t V = (size_t)d.V, F = (size_t)d.F;
    const Range ranges[6] = {{vertices, V * 12, 4},
                             {faces, F * 12, 4},
                             {sums, V * 24, 8},
                             {normals, V * 12, 4},
                             {scalars, 8 * LSF_MESH_SMOOTH_SCALAR_WORDS, 8},
                             {record, 8 * LSF_MESH_SMOOTH_RECORD_WORDS, 8}};
    if (!ranges_ok(ranges, 2)) return LSF_ERR_BAD_ARGUMENT;
    const int fresh = params->fresh_record;
    if (d.V == 0 && !fresh) return 0;
    d.vertices = vertices;
    d.faces = faces;
    d.degree = d.pinned = d.row = d.cursor = nullptr;
    d.keys = nullptr;
    d.counts = nullptr;
    d.offsets = nullptr;
    d.neighbours = nullptr;
    d.scalars = reinterpret_cast<unsigned long long*>(scalars);
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    LSF_SMOOTH_LAUNCH(normals_begin_kernel, 1, kWave, d, fresh);
    if (fresh && d.V > 0) LSF_SMOOTH_LAUNCH(validate_kernel, b.v, kBlock, d);
    if (d.F > 0 && (d.V > 0 || fresh)) LSF_SMOOTH_LAUNCH(normal_max_kernel, b.f, kBlock, d, fresh);
    if (d.V == 0) return 0;
    if (hipError_t e = hipMemsetAsync(sums, 0, V * 24, s)) return (int)e;
    if (d.F > 0)
        LSF_SMOOTH_LAUNCH(normal_scatter_kernel, b.f, kBlock, d, reinterpret_cast<unsigned long long*>(sums));
    LSF_SMOOTH_LAUNCH(normalise_kernel, b.v, kBlock, d, reinterpret_cast<const long long*>(sums), normals);
    return 0;
}
