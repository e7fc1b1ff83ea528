// Connected components of a triangle mesh and the filter that removes components (include/lsf_hip.h,
// lsf_mesh_components_label / _table / _select / _emit).  The contract is INTEGRATION.md section 3 ("Mesh components");
// tests/mesh_components_restatement.py restates it and the kernels equal it exactly, order included.
// Two vertices are connected when some face names both; a component's label is its smallest vertex index.
// The labels come from a lock-free union-find over parent[V]:
//   * parent[x] <= x always, and parent[x] == x makes x a root.  A root hi is linked under a smaller index lo of the other
//     set by atomicCAS(&parent[hi], hi, lo), and path halving lowers parent[x] of a non-root to one of x's ancestors by
//     atomicMin: a parent only ever moves to a strictly smaller index of the same set.  Every walk is therefore
//     strictly decreasing and ends, after at most V steps, at the smallest index its set has so far; when the linking
//     launch has ended the root of every vertex is its component's minimum, whichever lanes won.
//   * every read of parent[] inside the linking launch is a device-scope atomic load, or the value a failed
//     compare-and-swap returned: a plain load may be served from a CU's L1 for as long as the launch runs.
//   * every walk and every retry loop carries a cap of V + 1 steps.  A walk is strictly decreasing (at most V steps);
//     a compare-and-swap fails only because another lane's link succeeded, and at most V - 1 links ever succeed.  A
//     lane that reaches the cap adds to the record's step_cap word and stops; the wrapper raises on that word.
// The launch boundary makes all links visible: the flattening launch walks with plain loads and writes the labels to
// a plane of their own.  Counts and bounds are integer atomics into V-sized arrays indexed by label (the bounds through
// an order-preserving integer image of the float bits), added once per wave and label.  Rows of the table, kept
// vertices and kept faces come from tile-count scans over index order, so no output depends on the order lanes ran in
// or on the launch shape.  No float atomics, no inter-workgroup waits.
// Every launch but the one-workgroup scan walks tiles of LSF_MESH_COMPONENTS_TILE = 256 consecutive items, one per lane,
// on a grid capped at params.max_blocks (at most LSF_MESH_COMPONENTS_MAX_BLOCKS) workgroups with a stride loop behind it.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kTile = LSF_MESH_COMPONENTS_TILE;
constexpr int kScanThreads = LSF_MESH_COMPONENTS_SCAN_THREADS;
constexpr int kWaves = kBlock / kWave;
static_assert(kTile == kBlock, "one item per lane");

enum Field {
    kVerticesIn, kFacesIn, kInvalidVertices, kInvalidFaces, kComponents, kStepCap, kComponentsKept, kVerticesOut,
    kFacesOut
};
static_assert(kFacesOut + 1 == LSF_MESH_COMPONENTS_RECORD_WORDS, "the record's fields");

struct Dev {
    int V, F;
    long long cap;  // V + 1: the step cap of every walk and retry loop
    int tiles_v, tiles_f;
    // inputs
    const float* __restrict__ vertices;
    const int* __restrict__ faces;
    // workspaces: planes of vertex_work
    int *parent, *label, *vcount, *fcount;
    unsigned *lo, *hi;  // [3][V] each: the images of the bounds, indexed by label
    int *crow, *vout;
    // tile_offsets
    int *off_root, *off_kv, *off_kf;
    unsigned* stat_kept;
    unsigned long long* record;
};
static_assert(LSF_MESH_COMPONENTS_VERTEX_WORDS == 12, "parent, label, two counts, six bounds, row, output index");

// an unsigned integer that orders as the float does (-0 read as +0 first), and back
__device__ inline unsigned image_of(float p) {
    unsigned bits = __float_as_uint(p);
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}

__device__ inline float float_of(unsigned image) {
    return __uint_as_float((image & 0x80000000u) ? image & 0x7fffffffu : ~image);
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

// the number of set flags in the lanes below this one; every lane of the workgroup calls it
__device__ inline unsigned block_rank(bool flag) {
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const unsigned long long m = __ballot(flag);
    unsigned prefix = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();  // the words of the call before are read
    if (lane == 0) sh[wave] = (unsigned)__popcll(m);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) prefix += w < wave ? sh[w] : 0u;
    return prefix;
}

__global__ void begin_kernel(Dev d) {
    if (threadIdx.x < LSF_MESH_COMPONENTS_RECORD_WORDS)
        d.record[threadIdx.x] = threadIdx.x == kVerticesIn ? (unsigned long long)d.V
                                : threadIdx.x == kFacesIn  ? (unsigned long long)d.F
                                                           : 0ull;
}

__global__ __launch_bounds__(kBlock) void init_kernel(Dev d) {
    unsigned bad = 0;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ok = ok && isfinite(d.vertices[i * 3 + a]);
            d.lo[(long long)a * d.V + i] = 0xffffffffu;
            d.hi[(long long)a * d.V + i] = 0u;
        }
        d.parent[i] = (int)i;
        d.vcount[i] = 0;
        d.fcount[i] = 0;
        bad += ok ? 0u : 1u;
    }
    const unsigned total = block_sum(bad);
    if (threadIdx.x == 0 && total) atomicAdd(d.record + kInvalidVertices, (unsigned long long)total);
}

__device__ inline int load_parent(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root x's set had at some moment of the walk, or -1 at the step cap.  Path halving on the way: g is an ancestor of
// x with g < p < x, so the atomicMin keeps "a parent is a strictly smaller index of the same set".
__device__ inline int find_root(int* parent, int x, long long cap) {
    for (long long step = 0; step < cap; ++step) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        const int g = load_parent(parent, p);
        if (g != p) atomicMin(&parent[x], g);
        x = g;
    }
    return -1;
}

// the sets of a and b become one; false at a step cap
__device__ inline bool unite(int* parent, int a, int b, long long cap) {
    int ra = find_root(parent, a, cap), rb = find_root(parent, b, cap);
    for (long long retry = 0; retry < cap; ++retry) {
        if (ra < 0 || rb < 0) return false;
        if (ra == rb) return true;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return true;
        // another lane linked hi first: go on from the parent the failed compare-and-swap returned (old < hi)
        ra = find_root(parent, old, cap);
        rb = lo;
    }
    return false;
}

__global__ __launch_bounds__(kBlock) void link_kernel(Dev d) {
    unsigned bad = 0;
    bool capped = false;
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        if (f >= d.F) continue;
        const int a = d.faces[f * 3], b = d.faces[f * 3 + 1], c = d.faces[f * 3 + 2];
        if ((unsigned)a >= (unsigned)d.V || (unsigned)b >= (unsigned)d.V || (unsigned)c >= (unsigned)d.V) {
            ++bad;  // before any gather
            continue;
        }
        if (b != a && !unite(d.parent, a, b, d.cap)) capped = true;
        if (c != a && c != b && !unite(d.parent, a, c, d.cap)) capped = true;
    }
    if (capped) atomicAdd(d.record + kStepCap, 1ull);
    const unsigned total = block_sum(bad);
    if (threadIdx.x == 0 && total) atomicAdd(d.record + kInvalidFaces, (unsigned long long)total);
}

// Every lane of the wave calls it.  The lanes that share a label add their members and bounds to the label's words
// with one atomic per word: a mesh's neighbours in index order mostly share a component, and millions of atomics on one
// component's words would serialise.  At most kWave trips: each retires one label.
__device__ inline void add_members(const Dev& d, bool active, int label, const unsigned (&image)[3]) {
    const int lane = threadIdx.x % kWave;
    bool pending = active;
    for (int trip = 0; trip < kWave; ++trip) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader, kWave);
        const bool mine = pending && label == l;
        const int n = __popcll(__ballot(mine));  // wave-uniform
        unsigned lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = mine ? image[a] : 0xffffffffu;
            hi[a] = mine ? image[a] : 0u;
        }
        if (n > 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int s = kWave / 2; s > 0; s /= 2) {
                    lo[a] = min(lo[a], (unsigned)__shfl_xor(lo[a], s, kWave));
                    hi[a] = max(hi[a], (unsigned)__shfl_xor(hi[a], s, kWave));
                }
        }
        if (lane == leader) {
            atomicAdd(&d.vcount[l], n);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&d.lo[(long long)a * d.V + l], lo[a]);
                atomicMax(&d.hi[(long long)a * d.V + l], hi[a]);
            }
        }
        pending = pending && !mine;
    }
}

__device__ inline void add_faces(const Dev& d, bool active, int label) {
    const int lane = threadIdx.x % kWave;
    bool pending = active;
    for (int trip = 0; trip < kWave; ++trip) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader, kWave);
        const bool mine = pending && label == l;
        const int n = __popcll(__ballot(mine));
        if (lane == leader) atomicAdd(&d.fcount[l], n);
        pending = pending && !mine;
    }
}

// after the linking launch: plain loads.  The walk is strictly decreasing, so the cap is never reached on the parents
// the linking launch leaves; it is there for workspaces that are not its.
__global__ __launch_bounds__(kBlock) void flatten_kernel(Dev d) {
    bool capped = false;
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const bool in = i < d.V;
        int x = in ? (int)i : 0;
        bool found = !in;
        if (in) {
            for (long long step = 0; step < d.cap; ++step) {
                const int p = d.parent[x];
                if (p == x || (unsigned)p >= (unsigned)d.V) {
                    found = true;
                    break;
                }
                x = p;
            }
            d.label[i] = x;
        }
        capped = capped || !found;
        // (a non-finite vertex is counted by init_kernel and the wrapper refuses the mesh: its image is never read)
        unsigned image[3] = {0u, 0u, 0u};
        if (in)
#pragma unroll
            for (int a = 0; a < 3; ++a) image[a] = image_of(d.vertices[i * 3 + a]);
        add_members(d, in, x, image);
        const unsigned roots = block_sum(in && x == (int)i ? 1u : 0u);
        if (threadIdx.x == 0) d.off_root[tile] = (int)roots;
    }
    if (capped) atomicAdd(d.record + kStepCap, 1ull);
}

__global__ __launch_bounds__(kBlock) void face_count_kernel(Dev d) {
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        bool ok = f < d.F;
        int l = 0;
        if (ok) {
            const int a = d.faces[f * 3], b = d.faces[f * 3 + 1], c = d.faces[f * 3 + 2];
            ok = (unsigned)a < (unsigned)d.V && (unsigned)b < (unsigned)d.V && (unsigned)c < (unsigned)d.V;
            if (ok) l = d.label[a];
            ok = ok && (unsigned)l < (unsigned)d.V;
        }
        add_faces(d, ok, l);
    }
}

// one workgroup: the tile counts become their exclusive prefix (in place; the total is at most V or F, below 2^31) and
// the total goes to the record; the per-tile statistics words behind `stats`, when given, are summed into their record
// field on the way.  `tiles` may exceed the lane count: the workgroup loops.
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int* __restrict__ a, int tiles,
                                                            unsigned long long* __restrict__ record, int field,
                                                            const unsigned* __restrict__ stats, int stat_field) {
    __shared__ long long sh[kScanThreads / kWave];
    __shared__ unsigned long long sh_stat[kScanThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    long long running = 0;
    unsigned long long stat = 0;
    for (int base = 0; base < tiles; base += kScanThreads) {
        const int idx = base + threadIdx.x;
        const long long x = idx < tiles ? a[idx] : 0;
        if (stats && idx < tiles) stat += stats[idx];
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
#pragma unroll
    for (int s = kWave / 2; s > 0; s /= 2) stat += shfl_down_u64(stat, s);
    if (lane == 0) sh_stat[wave] = stat;
    __syncthreads();
    if (threadIdx.x == 0) {
        record[field] = (unsigned long long)running;
        if (stats) {
            unsigned long long total = 0;
            for (int w = 0; w < kScanThreads / kWave; ++w) total += sh_stat[w];
            record[stat_field] = total;
        }
    }
}

__global__ __launch_bounds__(kBlock) void rows_kernel(Dev d) {
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const bool root = i < d.V && d.label[i] == (int)i;
        const unsigned row = (unsigned)d.off_root[tile] + block_rank(root);
        if (i < d.V) d.crow[i] = root ? (int)row : -1;
    }
}

__global__ __launch_bounds__(kBlock) void table_kernel(Dev d, int* __restrict__ labels, int* __restrict__ vertex_counts,
                                                       int* __restrict__ face_counts, float* __restrict__ bounds,
                                                       long long components) {
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        if (i >= d.V) continue;
        const long long row = d.crow[i];
        if (row < 0 || row >= components) continue;
        labels[row] = (int)i;
        vertex_counts[row] = d.vcount[i];
        face_counts[row] = d.fcount[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bounds[row * 6 + a] = float_of(d.lo[(long long)a * d.V + i]);
            bounds[row * 6 + 3 + a] = float_of(d.hi[(long long)a * d.V + i]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void face_labels_kernel(Dev d, int* __restrict__ face_labels) {
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        if (f >= d.F) continue;
        const int a = d.faces[f * 3];
        face_labels[f] = (unsigned)a < (unsigned)d.V ? d.label[a] : -1;
    }
}

// whether vertex v's component is kept; every index is checked before it is used
__device__ inline bool kept(const Dev& d, const int* __restrict__ keep, long long components, int v) {
    if ((unsigned)v >= (unsigned)d.V) return false;
    const int l = d.label[v];
    if ((unsigned)l >= (unsigned)d.V) return false;
    const long long row = d.crow[l];
    return row >= 0 && row < components && keep[row] != 0;
}

__global__ __launch_bounds__(kBlock) void mark_vertices_kernel(Dev d, const int* __restrict__ keep, long long components) {
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const bool k = i < d.V && kept(d, keep, components, (int)i);
        const unsigned total = block_sum(k ? 1u : 0u);
        const unsigned roots = block_sum(k && d.label[i] == (int)i ? 1u : 0u);
        if (threadIdx.x == 0) {
            d.off_kv[tile] = (int)total;
            d.stat_kept[tile] = roots;
        }
    }
}

__global__ __launch_bounds__(kBlock) void mark_faces_kernel(Dev d, const int* __restrict__ keep, long long components) {
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        const bool k = f < d.F && kept(d, keep, components, d.faces[f * 3]);
        const unsigned total = block_sum(k ? 1u : 0u);
        if (threadIdx.x == 0) d.off_kf[tile] = (int)total;
    }
}

__global__ __launch_bounds__(kBlock) void emit_vertices_kernel(Dev d, const int* __restrict__ keep,
                                                               const float* __restrict__ normals,
                                                               const unsigned char* __restrict__ colours,
                                                               float* __restrict__ out_vertices,
                                                               float* __restrict__ out_normals,
                                                               unsigned char* __restrict__ out_colours,
                                                               long long components, long long vertices_out) {
    for (int tile = blockIdx.x; tile < d.tiles_v; tile += gridDim.x) {
        const long long i = (long long)tile * kTile + threadIdx.x;
        const bool k = i < d.V && kept(d, keep, components, (int)i);
        const long long row = (long long)d.off_kv[tile] + block_rank(k);
        if (i >= d.V) continue;
        const bool out = k && row < vertices_out;
        d.vout[i] = out ? (int)row : -1;
        if (!out) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out_vertices[row * 3 + a] = d.vertices[i * 3 + a];
            if (normals) out_normals[row * 3 + a] = normals[i * 3 + a];
            if (colours) out_colours[row * 3 + a] = colours[i * 3 + a];
        }
    }
}

__global__ __launch_bounds__(kBlock) void emit_faces_kernel(Dev d, const int* __restrict__ keep,
                                                            int* __restrict__ out_faces, long long components,
                                                            long long faces_out) {
    for (int tile = blockIdx.x; tile < d.tiles_f; tile += gridDim.x) {
        const long long f = (long long)tile * kTile + threadIdx.x;
        const bool k = f < d.F && kept(d, keep, components, d.faces[f * 3]);
        const long long row = (long long)d.off_kf[tile] + block_rank(k);
        if (!k || row >= faces_out) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int v = d.faces[f * 3 + a];  // in range: the labelling call refused the mesh otherwise
            out_faces[row * 3 + a] = (unsigned)v < (unsigned)d.V ? d.vout[v] : -1;
        }
    }
}

int tiles_of(long long n) { return (int)((n + kTile - 1) / kTile); }

struct Range {
    const void* p;
    size_t bytes;
};

// a buffer of a size that is not 0 must be given, on its alignment; no written buffer overlaps any other
template <int N>
bool ranges_ok(const Range (&r)[N], int first_written) {
    for (int i = 0; i < N; ++i)
        if (r[i].bytes && (!r[i].p || ((uintptr_t)r[i].p & 3) != 0)) return false;
    for (int i = first_written; i < N; ++i)
        for (int j = 0; j < i; ++j)
            if (overlaps(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) return false;
    return true;
}

// the checks every entry point shares, and the workspaces cut into their planes
int convert(const lsf_mesh_components_params* q, Dev& d, int& blocks_v, int& blocks_f) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->vertex_count < 0 || q->vertex_count > LSF_MESH_COMPONENTS_MAX_ITEMS || q->face_count < 0 ||
        q->face_count > LSF_MESH_COMPONENTS_MAX_ITEMS)
        return LSF_ERR_BAD_ARGUMENT;
    if (q->max_blocks < 0 || q->max_blocks > LSF_MESH_COMPONENTS_MAX_BLOCKS) return LSF_ERR_BAD_ARGUMENT;
    for (int flag : {q->has_normals, q->has_colours})
        if (flag != 0 && flag != 1) return LSF_ERR_BAD_ARGUMENT;
    d.V = q->vertex_count;
    d.F = q->face_count;
    d.cap = (long long)d.V + 1;
    d.tiles_v = tiles_of(d.V);
    d.tiles_f = tiles_of(d.F);
    const int most = q->max_blocks ? q->max_blocks : LSF_MESH_COMPONENTS_MAX_BLOCKS;
    blocks_v = d.tiles_v < most ? d.tiles_v : most;
    blocks_f = d.tiles_f < most ? d.tiles_f : most;
    return 0;
}

void cut(Dev& d, int32_t* vertex_work, int32_t* tile_offsets) {
    const long long V = d.V;
    d.parent = vertex_work;
    d.label = vertex_work + V;
    d.vcount = vertex_work + 2 * V;
    d.fcount = vertex_work + 3 * V;
    d.lo = reinterpret_cast<unsigned*>(vertex_work + 4 * V);
    d.hi = reinterpret_cast<unsigned*>(vertex_work + 7 * V);
    d.crow = vertex_work + 10 * V;
    d.vout = vertex_work + 11 * V;
    d.off_root = tile_offsets;
    d.off_kv = tile_offsets + d.tiles_v;
    d.stat_kept = reinterpret_cast<unsigned*>(tile_offsets + 2 * d.tiles_v);
    d.off_kf = tile_offsets + 3 * d.tiles_v;
}

size_t tile_words(const Dev& d) { return (size_t)(3 * d.tiles_v + d.tiles_f); }

}  // namespace

#define LSF_COMPONENTS_LAUNCH(kernel, blocks, threads, ...)                                 \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);         \
        if (int e = launch_status()) return e;                                              \
    } while (0)

extern "C" int lsf_mesh_components_label(const float* vertices, const int32_t* faces, int32_t* vertex_work,
                                         int32_t* tile_offsets, int64_t* record,
                                         const lsf_mesh_components_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    int bv, bf;
    if (int e = convert(params, d, bv, bf)) return e;
    if (!record || ((uintptr_t)record & 7) != 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t V = (size_t)d.V, F = (size_t)d.F;
    const Range ranges[5] = {{vertices, V * 12},
                             {faces, F * 12},
                             {vertex_work, V * 4 * LSF_MESH_COMPONENTS_VERTEX_WORDS},
                             {tile_offsets, tile_words(d) * 4},
                             {record, 8 * LSF_MESH_COMPONENTS_RECORD_WORDS}};
    if (!ranges_ok(ranges, 2)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, vertex_work, tile_offsets);
    d.vertices = vertices;
    d.faces = faces;
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    LSF_COMPONENTS_LAUNCH(begin_kernel, 1, kWave, d);
    if (d.V > 0) LSF_COMPONENTS_LAUNCH(init_kernel, bv, kBlock, d);
    if (d.F > 0) LSF_COMPONENTS_LAUNCH(link_kernel, bf, kBlock, d);
    if (d.V > 0) {
        LSF_COMPONENTS_LAUNCH(flatten_kernel, bv, kBlock, d);
        if (d.F > 0) LSF_COMPONENTS_LAUNCH(face_count_kernel, bf, kBlock, d);
        LSF_COMPONENTS_LAUNCH(scan_kernel, 1, kScanThreads, d.off_root, d.tiles_v, d.record, (int)kComponents,
                              (const unsigned*)nullptr, 0);
        LSF_COMPONENTS_LAUNCH(rows_kernel, bv, kBlock, d);
    }
    return 0;
}

extern "C" int lsf_mesh_components_table(const int32_t* faces, const int32_t* vertex_work, int32_t* labels,
                                         int32_t* vertex_counts, int32_t* face_counts, float* bounds,
                                         int32_t* face_labels, int64_t components,
                                         const lsf_mesh_components_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    int bv, bf;
    if (int e = convert(params, d, bv, bf)) return e;
    if (components < 0 || components > d.V || (d.V > 0 && components == 0)) return LSF_ERR_BAD_ARGUMENT;
    const size_t V = (size_t)d.V, F = (size_t)d.F, C = (size_t)components;
    const Range ranges[7] = {{faces, F * 12},
                             {vertex_work, V * 4 * LSF_MESH_COMPONENTS_VERTEX_WORDS},
                             {labels, C * 4},
                             {vertex_counts, C * 4},
                             {face_counts, C * 4},
                             {bounds, C * 24},
                             {face_labels, F * 4}};
    if (!ranges_ok(ranges, 2)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, const_cast<int32_t*>(vertex_work), nullptr);
    d.vertices = nullptr;
    d.faces = faces;
    d.record = nullptr;
    hipStream_t s = as_stream(stream);
    if (d.V > 0)
        LSF_COMPONENTS_LAUNCH(table_kernel, bv, kBlock, d, labels, vertex_counts, face_counts, bounds,
                              (long long)components);
    if (d.F > 0) LSF_COMPONENTS_LAUNCH(face_labels_kernel, bf, kBlock, d, face_labels);
    return 0;
}

extern "C" int lsf_mesh_components_select(const int32_t* faces, const int32_t* vertex_work, const int32_t* keep,
                                          int32_t* tile_offsets, int64_t* record, int64_t components,
                                          const lsf_mesh_components_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    int bv, bf;
    if (int e = convert(params, d, bv, bf)) return e;
    if (components < 0 || components > d.V || (d.V > 0 && components == 0)) return LSF_ERR_BAD_ARGUMENT;
    if (!record || ((uintptr_t)record & 7) != 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t V = (size_t)d.V, F = (size_t)d.F, C = (size_t)components;
    const Range ranges[5] = {{faces, F * 12},
                             {vertex_work, V * 4 * LSF_MESH_COMPONENTS_VERTEX_WORDS},
                             {keep, C * 4},
                             {tile_offsets, tile_words(d) * 4},
                             {record, 8 * LSF_MESH_COMPONENTS_RECORD_WORDS}};
    if (!ranges_ok(ranges, 3)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, const_cast<int32_t*>(vertex_work), tile_offsets);
    d.vertices = nullptr;
    d.faces = faces;
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    // components_kept, vertices_out, faces_out: zero where no scan below writes them
    if (hipError_t e = hipMemsetAsync(record + kComponentsKept, 0, 8 * 3, s)) return (int)e;
    if (d.V > 0) {
        LSF_COMPONENTS_LAUNCH(mark_vertices_kernel, bv, kBlock, d, keep, (long long)components);
        LSF_COMPONENTS_LAUNCH(scan_kernel, 1, kScanThreads, d.off_kv, d.tiles_v, d.record, (int)kVerticesOut,
                              (const unsigned*)d.stat_kept, (int)kComponentsKept);
    }
    if (d.V > 0 && d.F > 0) {
        LSF_COMPONENTS_LAUNCH(mark_faces_kernel, bf, kBlock, d, keep, (long long)components);
        LSF_COMPONENTS_LAUNCH(scan_kernel, 1, kScanThreads, d.off_kf, d.tiles_f, d.record, (int)kFacesOut,
                              (const unsigned*)nullptr, 0);
    }
    return 0;
}

extern "C" int lsf_mesh_components_emit(const float* vertices, const int32_t* faces, const float* normals,
                                        const uint8_t* colours, int32_t* vertex_work, const int32_t* keep,
                                        const int32_t* tile_offsets, float* out_vertices, float* out_normals,
                                        uint8_t* out_colours, int32_t* out_faces, int64_t components,
                                        int64_t vertices_out, int64_t faces_out,
                                        const lsf_mesh_components_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    int bv, bf;
    if (int e = convert(params, d, bv, bf)) return e;
    if (components < 0 || components > d.V || vertices_out < 0 || vertices_out > d.V || faces_out < 0 ||
        faces_out > d.F || (faces_out > 0 && vertices_out == 0))
        return LSF_ERR_BAD_ARGUMENT;
    if (vertices_out == 0) return 0;
    const bool has_normals = params->has_normals != 0, has_colours = params->has_colours != 0;
    if ((normals != nullptr) != has_normals || (out_normals != nullptr) != has_normals ||
        (colours != nullptr) != has_colours || (out_colours != nullptr) != has_colours)
        return LSF_ERR_BAD_ARGUMENT;
    const size_t V = (size_t)d.V, F = (size_t)d.F, C = (size_t)components, out = (size_t)vertices_out;
    // (colours are bytes: they are listed last, behind the ranges whose alignment is checked, and checked for NULL above)
    const Range ranges[9] = {{vertices, V * 12},
                             {faces, F * 12},
                             {normals, has_normals ? V * 12 : 0},
                             {keep, C * 4},
                             {tile_offsets, tile_words(d) * 4},
                             {vertex_work, V * 4 * LSF_MESH_COMPONENTS_VERTEX_WORDS},
                             {out_vertices, out * 12},
                             {out_normals, has_normals ? out * 12 : 0},
                             {out_faces, (size_t)faces_out * 12}};
    if (!ranges_ok(ranges, 5)) return LSF_ERR_BAD_ARGUMENT;
    if (has_colours) {
        for (int i = 0; i < 9; ++i)
            if (overlaps(out_colours, out * 3, ranges[i].p, ranges[i].bytes)) return LSF_ERR_BAD_ARGUMENT;
        for (int i = 5; i < 9; ++i)
            if (overlaps(colours, V * 3, ranges[i].p, ranges[i].bytes)) return LSF_ERR_BAD_ARGUMENT;
        if (overlaps(colours, V * 3, out_colours, out * 3)) return LSF_ERR_BAD_ARGUMENT;
    }
    cut(d, vertex_work, const_cast<int32_t*>(tile_offsets));
    d.vertices = vertices;
    d.faces = faces;
    d.record = nullptr;
    hipStream_t s = as_stream(stream);
    LSF_COMPONENTS_LAUNCH(emit_vertices_kernel, bv, kBlock, d, keep, normals, colours, out_vertices, out_normals,
                          out_colours, (long long)components, (long long)vertices_out);
    if (faces_out > 0)
        LSF_COMPONENTS_LAUNCH(emit_faces_kernel, bf, kBlock, d, keep, out_faces, (long long)components,
                              (long long)faces_out);
    return 0;
}
