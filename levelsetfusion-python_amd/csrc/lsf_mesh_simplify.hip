// Welding and vertex-clustering decimation of a triangle mesh (include/lsf_hip.h, lsf_mesh_simplify_count /
// lsf_mesh_simplify_emit).  The contract is INTEGRATION.md section 3 ("Mesh simplification");
// tests/mesh_simplify_restatement.py restates it and the kernels equal it exactly, order included.  Every float step is
// one float64 operation in the order written there (-ffp-contract=off); every sum is an integer atomic.
// One workgroup of 256 lanes owns one tile of LSF_MESH_SIMPLIFY_TILE = 256 consecutive items, one per lane; no grid is
// capped.  The launches of a call, in stream order:
//   count: begin        the record: the two input sizes, zeros
//          vertex key   per vertex its key (bit patterns, or lattice cell) and whether it is valid
//          vertex insert  each valid vertex finds the slot of its key in the hash table: it claims an empty slot by a
//                       compare-and-swap of its own index, or meets a slot whose holder has its key and lowers the
//                       holder to itself by atomicMin -- every holder a slot ever has carries the slot's one key, so
//                       the comparison gives the same answer whoever holds it, and at the end the holder is the
//                       cluster's smallest member
//          vertex first, scan, vertex id   "I am my slot's holder" scanned over the vertices: cluster ids in the order
//                       of the first members
//          accumulate   every vertex takes its cluster's id from the first member and adds its q, m and colour
//          face key     per face the bounds check, the cluster ids, invalid / degenerate, the sorted triple and the sign
//          face insert  the same table, refilled: the claimer of a slot stays, and names the group; the group's net sign
//                       by atomicAdd and the first face of each orientation by atomicMin
//          face select, scan   the face that survives per group, the clusters it uses, the group statistics (per
//                       tile, summed into the record by the scan, as the invalid and degenerate counts are)
//          cluster used, scan  the clusters some surviving face references, counted per tile
//   (the host reads the record and allocates the outputs)
//   emit:  vertices     a ballot scan gives each used cluster its output row; position, normal and colour written
//          faces        a ballot scan gives each surviving face its row; indices remapped, winding kept
// Which lane claims a slot is a race and so is the slot a key ends in; neither reaches an output: ids come from scans
// over index order, sums are integers, minima are minima.  A key's launch ends before the launch that compares keys
// begins, so a claimer's key is visible to the lane that lost to it.
#include "lsf_device.h"

using namespace lsf;

namespace {

constexpr int kTile = LSF_MESH_SIMPLIFY_TILE;
constexpr int kScanThreads = LSF_MESH_SIMPLIFY_SCAN_THREADS;
constexpr int kWaves = kBlock / kWave;
static_assert(kTile == kBlock, "one item per lane");

enum Field {
    kVerticesIn, kFacesIn, kInvalidVertices, kInvalidFaces, kClusters, kDegenerateFaces, kFaceGroups, kCancelledGroups,
    kMultiCoverGroups, kOrphanClusters, kVerticesOut, kFacesOut, kTableOverflow
};
static_assert(kTableOverflow + 1 == LSF_MESH_SIMPLIFY_RECORD_WORDS, "the record's fields");

constexpr double kQOne = 16777216.0;        // 2^24 quantisation bins per cell and axis
constexpr double kMaxCell = 1048576.0;      // |c| beyond 2^20 is invalid
constexpr double kNormalOne = 1073741824.0; // 2^30
constexpr double kNormalClamp = 2.0;

// face states between the face launches
constexpr int kFaceInvalid = -1, kFaceDegenerate = -2, kFaceOverflow = -3;

struct Dev {
    double cell, origin[3];
    int V, F;
    unsigned slots, mask;
    int cluster, has_normals, has_colours;
    int K, normal_at, colour_at;  // int64 words per row of sums, and where the normal and colour sums begin
    // inputs
    const float* __restrict__ vertices;
    const int* __restrict__ faces;
    const float* __restrict__ normals;
    const unsigned char* __restrict__ colours;
    // workspaces
    int* table;
    int *vkey, *vslot, *vcluster;
    int *ccount, *cused, *cfirst, *cout;
    unsigned long long* sums;
    int *fkey, *fstate, *fnet;
    unsigned *fmin_pos, *fmin_neg;
    int *off_v, *off_c, *off_f;
    unsigned *stat_v, *stat_key, *stat_select;  // per tile, three 10-bit counts in a word: summed by the scans
    unsigned long long* record;
};

__device__ inline unsigned hash3(unsigned a, unsigned b, unsigned c) {
    unsigned h = a * 0x9E3779B1u;
    h = (h ^ (h >> 15)) + b * 0x85EBCA77u;
    h = (h ^ (h >> 13)) + c * 0xC2B2AE3Du;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    return h ^ (h >> 16);
}

// the cell c and the bin q of one coordinate
__device__ inline void cell_of(float p, double origin, double cell, double& c, long long& q) {
    const double r = ((double)p - origin) / cell;
    c = floor(r);
    const double fq = floor((r - c) * kQOne);
    q = fq < kQOne - 1.0 ? (long long)fq : (long long)(kQOne - 1.0);
}

__device__ inline unsigned block_sum(unsigned value) {
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int d = kWave / 2; d > 0; d /= 2) value += __shfl_xor(value, d, kWave);
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
    if (lane == 0) sh[wave] = (unsigned)__popcll(m);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) prefix += w < wave ? sh[w] : 0u;
    return prefix;
}

__global__ void begin_kernel(Dev d) {
    if (threadIdx.x < LSF_MESH_SIMPLIFY_RECORD_WORDS)
        d.record[threadIdx.x] = threadIdx.x == kVerticesIn ? (unsigned long long)d.V
                                : threadIdx.x == kFacesIn  ? (unsigned long long)d.F
                                                           : 0ull;
}

__global__ __launch_bounds__(kBlock) void vertex_key_kernel(Dev d) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned bad = 0;
    if (i < d.V) {
        bool ok = true;
        int k[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p = d.vertices[i * 3 + a];
            ok = ok && isfinite(p);
            if (d.cluster) {
                double c;
                long long q;
                cell_of(p, d.origin[a], d.cell, c, q);
                const bool in = fabs(c) <= kMaxCell;  // false for an overflow to inf and for a NaN
                ok = ok && in;
                k[a] = in ? (int)c : 0;
            } else {
                const unsigned bits = __float_as_uint(p);
                k[a] = (int)(bits == 0x80000000u ? 0u : bits);
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) d.vkey[i * 3 + a] = k[a];
        d.vslot[i] = ok ? 0 : -1;
        bad = ok ? 0u : 1u;
    }
    const unsigned total = block_sum(bad);
    if (threadIdx.x == 0) d.stat_v[blockIdx.x] = total;
}

// the slot of item i's key: claimed, or met with an equal key.  At most `slots` probes; -1 when the table is full.
// `claimed` tells which; `holder` is the index the slot held when it was met.
__device__ inline int find_slot(int* table, const int* __restrict__ keys, int count, int i, unsigned slots,
                                unsigned mask, bool& claimed, int& holder) {
    const int k0 = keys[(long long)i * 3], k1 = keys[(long long)i * 3 + 1], k2 = keys[(long long)i * 3 + 2];
    unsigned h = hash3((unsigned)k0, (unsigned)k1, (unsigned)k2) & mask;
    claimed = false;
    holder = i;
    for (unsigned n = 0; n < slots; ++n) {
        const int cur = atomicCAS(&table[h], -1, i);
        if (cur == -1) {
            claimed = true;
            return (int)h;
        }
        if ((unsigned)cur < (unsigned)count) {  // (the table holds nothing else)
            const long long at = (long long)cur * 3;
            if (keys[at] == k0 && keys[at + 1] == k1 && keys[at + 2] == k2) {
                holder = cur;
                return (int)h;
            }
        }
        h = (h + 1u) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void vertex_insert_kernel(Dev d) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.V || d.vslot[i] < 0) return;
    bool claimed;
    int holder;
    const int slot = find_slot(d.table, d.vkey, d.V, (int)i, d.slots, d.mask, claimed, holder);
    if (slot < 0) atomicAdd(d.record + kTableOverflow, 1ull);
    else if (!claimed) atomicMin(&d.table[slot], (int)i);
    d.vslot[i] = slot;
}

__device__ inline bool is_first(const Dev& d, long long i) {
    if (i >= d.V) return false;
    const int slot = d.vslot[i];
    return slot >= 0 && d.table[slot] == (int)i;
}

__global__ __launch_bounds__(kBlock) void vertex_first_kernel(Dev d) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned total = block_sum(is_first(d, i) ? 1u : 0u);
    if (threadIdx.x == 0) d.off_v[blockIdx.x] = (int)total;
}

// the record fields that the three 10-bit counts of a plane of per-tile words add up to; -1: none
struct StatFields {
    int field[2][3];
};

// one workgroup: the tile counts become their exclusive prefix (in place; the host bounds the total below 2^31) and
// the total goes to the record; the `planes` planes of per-tile statistics words behind `stats` are summed into their
// record fields on the way (a tile's workgroup adding to the record itself would be tens of thousands of atomics on one
// address).  `blocks` may exceed the lane count: the workgroup loops.
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int* __restrict__ a, int blocks,
                                                            unsigned long long* __restrict__ record, int field,
                                                            const unsigned* __restrict__ stats, int planes,
                                                            StatFields fields) {
    __shared__ long long sh[kScanThreads / kWave];
    __shared__ unsigned long long sh_stat[2][3][kScanThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    long long running = 0;
    unsigned long long stat[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (int base = 0; base < blocks; base += kScanThreads) {
        const int idx = base + threadIdx.x;
        const long long x = idx < blocks ? a[idx] : 0;
        for (int p = 0; p < planes; ++p) {
            const unsigned w = idx < blocks ? stats[(long long)p * blocks + idx] : 0u;
            stat[p][0] += w & 1023u;
            stat[p][1] += (w >> 10) & 1023u;
            stat[p][2] += w >> 20;
        }
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
        if (idx < blocks) a[idx] = (int)(running + before + incl - x);
        running += step;
        __syncthreads();  // sh is rewritten by the next step
    }
    for (int p = 0; p < planes; ++p)
        for (int k = 0; k < 3; ++k) {
            unsigned long long v = stat[p][k];
#pragma unroll
            for (int s = kWave / 2; s > 0; s /= 2) v += shfl_down_u64(v, s);
            if (lane == 0) sh_stat[p][k][wave] = v;
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        record[field] = (unsigned long long)running;
        if (field == kVerticesOut) record[kOrphanClusters] = record[kClusters] - (unsigned long long)running;
        for (int p = 0; p < planes; ++p)
            for (int k = 0; k < 3; ++k) {
                if (fields.field[p][k] < 0) continue;
                unsigned long long total = 0;
                for (int w = 0; w < kScanThreads / kWave; ++w) total += sh_stat[p][k][w];
                record[fields.field[p][k]] = total;
            }
    }
}

__global__ __launch_bounds__(kBlock) void vertex_id_kernel(Dev d) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool first = is_first(d, i);
    const unsigned rank = (unsigned)d.off_v[blockIdx.x] + block_rank(first);
    if (i >= d.V) return;
    if (first) {
        d.vcluster[i] = (int)rank;
        d.cfirst[rank] = (int)i;
    } else if (d.vslot[i] < 0) {
        d.vcluster[i] = -1;
    }
}

__global__ __launch_bounds__(kBlock) void accumulate_kernel(Dev d) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.V) return;
    const int slot = d.vslot[i];
    if (slot < 0) return;
    const int first = d.table[slot];
    const int cid = d.vcluster[first];  // written by the launch before, for first members only
    if (first != (int)i) d.vcluster[i] = cid;  // (read by this lane alone until the launch ends)
    atomicAdd(&d.ccount[cid], 1);
    unsigned long long* row = d.sums + (long long)cid * d.K;
    if (d.cluster) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double c;
            long long q;
            cell_of(d.vertices[i * 3 + a], d.origin[a], d.cell, c, q);
            atomicAdd(row + a, (unsigned long long)q);
        }
    }
    if (d.has_normals) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = d.normals[i * 3 + a];
            const double v = isfinite(x) ? (double)x : 0.0;
            const long long m = llrint(fmin(fmax(v, -kNormalClamp), kNormalClamp) * kNormalOne);
            atomicAdd(row + d.normal_at + a, (unsigned long long)m);  // two's complement: a signed sum
        }
    }
    if (d.has_colours) {
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd(row + d.colour_at + a, (unsigned long long)d.colours[i * 3 + a]);
    }
}

__global__ __launch_bounds__(kBlock) void face_key_kernel(Dev d) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned counts = 0;  // invalid | degenerate << 10
    if (f < d.F) {
        int id[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int v = d.faces[f * 3 + a];
            const bool in = (unsigned)v < (unsigned)d.V;  // before the gather
            id[a] = in ? d.vcluster[v] : -1;
            ok = ok && id[a] >= 0;
        }
        int state;
        if (!ok) {
            state = kFaceInvalid;
            counts = 1u;
        } else if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) {
            state = kFaceDegenerate;
            counts = 1u << 10;
        } else {
            // begun at its smallest id the face is (lo, x, y): a rotation of the sorted triple when x < y
            const int lo = min(id[0], min(id[1], id[2])), hi = max(id[0], max(id[1], id[2]));
            const int at = id[0] == lo ? 0 : (id[1] == lo ? 1 : 2);
            const int x = id[(at + 1) % 3], y = id[(at + 2) % 3];
            d.fkey[f * 3] = lo;
            d.fkey[f * 3 + 1] = x < y ? x : y;
            d.fkey[f * 3 + 2] = hi;
            state = x < y ? 0 : 1;  // 1: the other orientation
        }
        d.fstate[f] = state;
    }
    const unsigned total = block_sum(counts);
    if (threadIdx.x == 0) d.stat_key[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void face_insert_kernel(Dev d) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (f >= d.F) return;
    const int neg = d.fstate[f];
    if (neg < 0) return;
    bool claimed;
    int group;
    const int slot = find_slot(d.table, d.fkey, d.F, (int)f, d.slots, d.mask, claimed, group);
    if (slot < 0) {
        atomicAdd(d.record + kTableOverflow, 1ull);
        d.fstate[f] = kFaceOverflow;
        return;
    }
    atomicAdd(&d.fnet[group], neg ? -1 : 1);
    atomicMin(&(neg ? d.fmin_neg : d.fmin_pos)[group], (unsigned)f);
    d.fstate[f] = 2 * group + neg;
}

__global__ __launch_bounds__(kBlock) void face_select_kernel(Dev d) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    unsigned counts = 0;  // groups | cancelled << 10 | multi cover << 20
    bool keep = false;
    if (f < d.F) {
        const int state = d.fstate[f];
        if (state >= 0) {
            const int group = state >> 1, neg = state & 1;
            const int net = d.fnet[group];
            if (group == (int)f) counts = 1u | (net == 0 ? 1u << 10 : 0u) | (net >= 2 || net <= -2 ? 1u << 20 : 0u);
            keep = net > 0 ? (!neg && d.fmin_pos[group] == (unsigned)f) : (net < 0 && neg && d.fmin_neg[group] == (unsigned)f);
            if (keep)
#pragma unroll
                for (int a = 0; a < 3; ++a) d.cused[d.fkey[f * 3 + a]] = 1;  // every writer stores the same word
        }
        d.fstate[f] = keep ? 1 : 0;
    }
    const unsigned kept = block_sum(keep ? 1u : 0u);
    __syncthreads();  // block_sum's words are rewritten
    const unsigned total = block_sum(counts);
    if (threadIdx.x == 0) {
        d.off_f[blockIdx.x] = (int)kept;
        d.stat_select[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kBlock) void cluster_used_kernel(Dev d) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long clusters = (long long)d.record[kClusters];
    const unsigned total = block_sum(c < clusters && c < d.V && d.cused[c] ? 1u : 0u);
    if (threadIdx.x == 0) d.off_c[blockIdx.x] = (int)total;
}

__global__ __launch_bounds__(kBlock) void emit_vertices_kernel(Dev d, float* __restrict__ out_vertices,
                                                               float* __restrict__ out_normals,
                                                               unsigned char* __restrict__ out_colours,
                                                               long long clusters, long long vertices_out) {
    const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool used = c < clusters && d.cused[c] != 0;
    const long long row = (long long)d.off_c[blockIdx.x] + block_rank(used);
    if (c >= clusters) return;
    d.cout[c] = used && row < vertices_out ? (int)row : -1;
    if (!used || row >= vertices_out) return;
    const int first = d.cfirst[c];
    if ((unsigned)first >= (unsigned)d.V) return;  // not lsf_mesh_simplify_count's workspaces
    const long long n = d.ccount[c];
    const unsigned long long* sums = d.sums + c * d.K;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = d.vertices[(long long)first * 3 + a];
        float out = p;
        if (d.cluster) {
            double cell;
            long long q;
            cell_of(p, d.origin[a], d.cell, cell, q);
            const double inside = ((double)(long long)sums[a] + 0.5 * (double)n) / ((double)n * kQOne);
            out = (float)(d.origin[a] + d.cell * (cell + inside));
        }
        out_vertices[row * 3 + a] = out;
    }
    if (d.has_normals) {
        double s[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] = (double)(long long)sums[d.normal_at + a];
        const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) out_normals[row * 3 + a] = len != 0.0 ? (float)(s[a] / len) : 0.0f;
    }
    if (d.has_colours) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long sum = sums[d.colour_at + a];
            out_colours[row * 3 + a] = n > 0 ? (unsigned char)((2ull * sum + (unsigned long long)n) / (2ull * (unsigned long long)n)) : 0;
        }
    }
}

__global__ __launch_bounds__(kBlock) void emit_faces_kernel(Dev d, int* __restrict__ out_faces, long long clusters,
                                                            long long faces_out) {
    const long long f = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool keep = f < d.F && d.fstate[f] == 1;
    const long long row = (long long)d.off_f[blockIdx.x] + block_rank(keep);
    if (!keep || row >= faces_out) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int v = d.faces[f * 3 + a];
        const int c = (unsigned)v < (unsigned)d.V ? d.vcluster[v] : -1;
        out_faces[row * 3 + a] = c >= 0 && c < clusters ? d.cout[c] : -1;
    }
}

int blocks_of(long long n) { return (int)((n + kTile - 1) / kTile); }

// the checks both entry points share, and the workspaces cut into their planes
int convert(const lsf_mesh_simplify_params* q, Dev& d) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->vertex_count < 0 || q->vertex_count > LSF_MESH_SIMPLIFY_MAX_ITEMS || q->face_count < 0 ||
        q->face_count > LSF_MESH_SIMPLIFY_MAX_ITEMS)
        return LSF_ERR_BAD_ARGUMENT;
    const long long most = q->vertex_count > q->face_count ? q->vertex_count : q->face_count;
    const long long slots = q->table_slots;
    if (slots < 2 || (slots & (slots - 1)) != 0 || slots < 2 * most) return LSF_ERR_BAD_ARGUMENT;
    for (int flag : {q->cluster, q->has_normals, q->has_colours})
        if (flag != 0 && flag != 1) return LSF_ERR_BAD_ARGUMENT;
    if (q->cluster) {
        for (double x : {q->cell_size, q->origin_x, q->origin_y, q->origin_z})
            if (!std::isfinite(x)) return LSF_ERR_BAD_ARGUMENT;
        if (!(q->cell_size > 0.0)) return LSF_ERR_BAD_ARGUMENT;
    }
    d.cell = q->cluster ? q->cell_size : 1.0;
    d.origin[0] = q->cluster ? q->origin_x : 0.0;
    d.origin[1] = q->cluster ? q->origin_y : 0.0;
    d.origin[2] = q->cluster ? q->origin_z : 0.0;
    d.V = q->vertex_count;
    d.F = q->face_count;
    d.slots = (unsigned)slots;
    d.mask = (unsigned)slots - 1u;
    d.cluster = q->cluster;
    d.has_normals = q->has_normals;
    d.has_colours = q->has_colours;
    d.normal_at = 3 * q->cluster;
    d.colour_at = d.normal_at + 3 * q->has_normals;
    d.K = d.colour_at + 3 * q->has_colours;
    return 0;
}

void cut(Dev& d, int32_t* table, int32_t* vertex_work, int32_t* cluster_work, int64_t* sums, int32_t* face_work,
         int32_t* tile_offsets) {
    const long long V = d.V, F = d.F;
    d.table = table;
    d.vkey = vertex_work;
    d.vslot = vertex_work + 3 * V;
    d.vcluster = vertex_work + 4 * V;
    d.ccount = cluster_work;
    d.cused = cluster_work + V;
    d.cfirst = cluster_work + 2 * V;
    d.cout = cluster_work + 3 * V;
    d.sums = reinterpret_cast<unsigned long long*>(sums);
    d.fkey = face_work;
    d.fstate = face_work + 3 * F;
    d.fnet = face_work + 4 * F;
    d.fmin_pos = reinterpret_cast<unsigned*>(face_work + 5 * F);
    d.fmin_neg = reinterpret_cast<unsigned*>(face_work + 6 * F);
    d.off_v = tile_offsets;
    d.off_c = tile_offsets + blocks_of(V);
    d.stat_v = reinterpret_cast<unsigned*>(tile_offsets + 2 * blocks_of(V));
    d.off_f = tile_offsets + 3 * blocks_of(V);
    d.stat_key = reinterpret_cast<unsigned*>(tile_offsets + 3 * blocks_of(V) + blocks_of(F));
    d.stat_select = reinterpret_cast<unsigned*>(tile_offsets + 3 * blocks_of(V) + 2 * blocks_of(F));
}

struct Range {
    const void* p;
    size_t bytes;
};

// a buffer of a size that is not 0 must be given; no written buffer overlaps any other
template <int N>
bool ranges_ok(const Range (&r)[N], int first_written) {
    for (int i = 0; i < N; ++i)
        if (r[i].bytes && !r[i].p) return false;
    for (int i = first_written; i < N; ++i)
        for (int j = 0; j < i; ++j)
            if (overlaps(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) return false;
    return true;
}

int fill(void* p, int value, size_t bytes, hipStream_t s) {
    if (!bytes) return 0;
    return (int)hipMemsetAsync(p, value, bytes, s);
}

}  // namespace

#define LSF_SIMPLIFY_LAUNCH(kernel, blocks, threads, ...)                                   \
    do {                                                                                    \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);         \
        if (int e = launch_status()) return e;                                              \
    } while (0)

extern "C" int lsf_mesh_simplify_count(const float* vertices, const int32_t* faces, const float* normals,
                                       const uint8_t* colours, int32_t* table, int32_t* vertex_work,
                                       int32_t* cluster_work, int64_t* sums, int32_t* face_work, int32_t* tile_offsets,
                                       int64_t* record, const lsf_mesh_simplify_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    if (int e = convert(params, d)) return e;
    if ((normals != nullptr) != (d.has_normals != 0) && d.V > 0) return LSF_ERR_BAD_ARGUMENT;
    if ((colours != nullptr) != (d.has_colours != 0) && d.V > 0) return LSF_ERR_BAD_ARGUMENT;
    if (!record) return LSF_ERR_BAD_ARGUMENT;
    const size_t V = (size_t)d.V, F = (size_t)d.F;
    const int bv = blocks_of(d.V), bf = blocks_of(d.F);
    const Range ranges[11] = {{vertices, V * 12},
                              {faces, F * 12},
                              {normals, d.has_normals ? V * 12 : 0},
                              {colours, d.has_colours ? V * 3 : 0},
                              {table, (size_t)d.slots * 4},
                              {vertex_work, V * 4 * LSF_MESH_SIMPLIFY_VERTEX_WORDS},
                              {cluster_work, V * 4 * LSF_MESH_SIMPLIFY_CLUSTER_WORDS},
                              {sums, V * 8 * (size_t)d.K},
                              {face_work, F * 4 * LSF_MESH_SIMPLIFY_FACE_WORDS},
                              {tile_offsets, (size_t)(3 * bv + 3 * bf) * 4},
                              {record, 8 * LSF_MESH_SIMPLIFY_RECORD_WORDS}};
    if (!ranges_ok(ranges, 4)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, table, vertex_work, cluster_work, sums, face_work, tile_offsets);
    d.vertices = vertices;
    d.faces = faces;
    d.normals = normals;
    d.colours = colours;
    d.record = reinterpret_cast<unsigned long long*>(record);
    hipStream_t s = as_stream(stream);
    LSF_SIMPLIFY_LAUNCH(begin_kernel, 1, kWave, d);
    if (d.V > 0) {
        if (int e = fill(d.table, 0xff, (size_t)d.slots * 4, s)) return e;
        if (int e = fill(d.ccount, 0, V * 8, s)) return e;  // members and used
        if (int e = fill(d.sums, 0, V * 8 * (size_t)d.K, s)) return e;
        LSF_SIMPLIFY_LAUNCH(vertex_key_kernel, bv, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(vertex_insert_kernel, bv, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(vertex_first_kernel, bv, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(scan_kernel, 1, kScanThreads, d.off_v, bv, d.record, (int)kClusters, d.stat_v, 1,
                            (StatFields{{{kInvalidVertices, -1, -1}, {-1, -1, -1}}}));
        LSF_SIMPLIFY_LAUNCH(vertex_id_kernel, bv, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(accumulate_kernel, bv, kBlock, d);
    }
    if (d.F > 0) {
        if (int e = fill(d.table, 0xff, (size_t)d.slots * 4, s)) return e;
        if (int e = fill(d.fnet, 0, F * 4, s)) return e;
        if (int e = fill(d.fmin_pos, 0xff, F * 8, s)) return e;  // both orientations
        LSF_SIMPLIFY_LAUNCH(face_key_kernel, bf, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(face_insert_kernel, bf, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(face_select_kernel, bf, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(scan_kernel, 1, kScanThreads, d.off_f, bf, d.record, (int)kFacesOut, d.stat_key, 2,
                            (StatFields{{{kInvalidFaces, kDegenerateFaces, -1},
                                         {kFaceGroups, kCancelledGroups, kMultiCoverGroups}}}));
    }
    if (d.V > 0) {
        LSF_SIMPLIFY_LAUNCH(cluster_used_kernel, bv, kBlock, d);
        LSF_SIMPLIFY_LAUNCH(scan_kernel, 1, kScanThreads, d.off_c, bv, d.record, (int)kVerticesOut,
                            (const unsigned*)nullptr, 0, (StatFields{{{-1, -1, -1}, {-1, -1, -1}}}));
    }
    return 0;
}

extern "C" int lsf_mesh_simplify_emit(const float* vertices, const int32_t* faces, const int32_t* vertex_work,
                                      int32_t* cluster_work, const int64_t* sums, const int32_t* face_work,
                                      const int32_t* tile_offsets, float* out_vertices, float* out_normals,
                                      uint8_t* out_colours, int32_t* out_faces, int64_t clusters, int64_t vertices_out,
                                      int64_t faces_out, const lsf_mesh_simplify_params* params, void* stream) {
    (void)hipGetLastError();
    Dev d;
    if (int e = convert(params, d)) return e;
    if (clusters < 0 || clusters > d.V || vertices_out < 0 || vertices_out > clusters || faces_out < 0 ||
        faces_out > d.F || (faces_out > 0 && vertices_out == 0))
        return LSF_ERR_BAD_ARGUMENT;
    if (vertices_out == 0) return 0;
    const size_t V = (size_t)d.V, F = (size_t)d.F, out = (size_t)vertices_out;
    const int bv = blocks_of(d.V), bf = blocks_of(d.F);
    if ((out_normals != nullptr) != (d.has_normals != 0) || (out_colours != nullptr) != (d.has_colours != 0))
        return LSF_ERR_BAD_ARGUMENT;
    const Range ranges[11] = {{vertices, V * 12},
                              {faces, F * 12},
                              {sums, V * 8 * (size_t)d.K},
                              {face_work, F * 4 * LSF_MESH_SIMPLIFY_FACE_WORDS},
                              {tile_offsets, (size_t)(3 * bv + 3 * bf) * 4},
                              {vertex_work, V * 4 * LSF_MESH_SIMPLIFY_VERTEX_WORDS},
                              {cluster_work, V * 4 * LSF_MESH_SIMPLIFY_CLUSTER_WORDS},
                              {out_vertices, out * 12},
                              {out_normals, d.has_normals ? out * 12 : 0},
                              {out_colours, d.has_colours ? out * 3 : 0},
                              {out_faces, (size_t)faces_out * 12}};
    if (!ranges_ok(ranges, 6)) return LSF_ERR_BAD_ARGUMENT;
    cut(d, nullptr, const_cast<int32_t*>(vertex_work), cluster_work, const_cast<int64_t*>(sums), const_cast<int32_t*>(face_work),
        const_cast<int32_t*>(tile_offsets));
    d.vertices = vertices;
    d.faces = faces;
    d.normals = nullptr;
    d.colours = nullptr;
    d.record = nullptr;
    hipStream_t s = as_stream(stream);
    LSF_SIMPLIFY_LAUNCH(emit_vertices_kernel, blocks_of(clusters), kBlock, d, out_vertices, out_normals, out_colours,
                        (long long)clusters, (long long)vertices_out);
    if (faces_out > 0)
        LSF_SIMPLIFY_LAUNCH(emit_faces_kernel, bf, kBlock, d, out_faces, (long long)clusters, (long long)faces_out);
    return 0;
}
