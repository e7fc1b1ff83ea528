// A triangle mesh of the canonical TSDF's level set (include/lsf_hip.h, lsf_mesh_count / lsf_mesh_emit): the model
// export of KillingFusion-style systems, which the reference does not have.  The contract is INTEGRATION.md section 3
// ("Mesh extraction"); tests/mesh_restatement.py restates it and the kernels equal it bit for bit, order included.
// Every float step is one float64 operation in the order written there; -ffp-contract=off keeps them separate.
// The case table is generated (tools/gen_mesh_tables.py -> lsf_mesh_tables.h).
// Five launches, each workgroup of 256 lanes owning one tile of LSF_MESH_TILE consecutive voxels (cells are named by
// their lowest voxel, so a tile is also a tile of cells), lane t taking voxels t, t + 256, ... of its tile:
//   count: classify   per cell its code (the case when valid, else 0) and the tile's triangle count
//          edges      per voxel the mask of its x, y, z grid edges that carry a vertex (from the <= 7 cells that hold
//                     them) and the tile's vertex count
//          scan       one workgroup: exclusive offsets of the tiles' counts, and the two totals
//   (the host reads the totals and allocates the outputs)
//   emit:  vertices   a ballot scan over the tile gives each voxel its first vertex; positions (and normals) written
//          faces      a ballot scan gives each cell its first face; each edge's vertex is
//                     vertex_base[owner] + popcount(edge_mask[owner] & ((1 << axis) - 1))
// The order of the outputs is the order of the voxels, whatever the schedule: no atomics between workgroups, no flags.
// lsf_mesh_vertex_colours is a sixth, optional launch after emit ("Colour fusion";
// tests/colour_restatement.py): every voxel that owns vertices interpolates their colours from a volume of float32
// (R, G, B, Wc) records with the vertices' own t and writes its rows from vertex_base; it needs no scan.
#include "lsf_device.h"
#include "lsf_mesh_tables.h"

using namespace lsf;

namespace {

constexpr int kTile = LSF_MESH_TILE;
constexpr int kSteps = kTile / kBlock;
constexpr int kWaves = kBlock / kWave;
constexpr int kScanThreads = 1024;
static_assert(kTile % kBlock == 0, "a tile is a whole number of workgroup steps");

struct MeshDev {
    double voxel, iso, min_weight;
    double off[3];
    int nx, ny, nz;
    long long voxels;
    int blocks;
};

struct Volume {
    const float* __restrict__ tsdf;
    const float* __restrict__ weight;
};

// (x, y, z) of voxel v in two 32-bit divisions: the host bounds the voxel count below 2^31
__device__ inline void coords(long long v, const MeshDev& p, int& x, int& y, int& z) {
    const unsigned u = (unsigned)v, row = u / (unsigned)p.nx;
    x = (int)(u - row * (unsigned)p.nx);
    z = (int)(row / (unsigned)p.ny);
    y = (int)(row - (unsigned)z * (unsigned)p.ny);
}

__device__ inline bool usable(const Volume& vol, long long v, const MeshDev& p) {
    return (double)vol.weight[v] > p.min_weight && isfinite(vol.tsdf[v]);  // NaN weights fail
}

// the wave's exclusive prefix and total of a per-lane count of `Bits` bits, from one ballot per bit
template <int Bits>
__device__ inline void wave_scan(unsigned value, int lane, unsigned& prefix, unsigned& total) {
    const unsigned long long below = (1ull << lane) - 1ull;
    prefix = 0;
    total = 0;
#pragma unroll
    for (int b = 0; b < Bits; ++b) {
        const unsigned long long m = __ballot((value >> b) & 1u);
        prefix += (unsigned)__popcll(m & below) << b;
        total += (unsigned)__popcll(m) << b;
    }
}

// one workgroup step of a tile: the lane's exclusive prefix within the step and the step's total
template <int Bits>
__device__ inline void block_scan(unsigned value, unsigned (&sh)[2][kWaves], int parity, unsigned& prefix,
                                  unsigned& total) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned wp, wt;
    wave_scan<Bits>(value, lane, wp, wt);
    if (lane == 0) sh[parity][wave] = wt;
    __syncthreads();  // (the other parity's slots are rewritten only after the next step's barrier)
    prefix = wp;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const unsigned t = sh[parity][w];
        prefix += w < wave ? t : 0u;
        total += t;
    }
}

__device__ inline int block_sum(unsigned value) {
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int d = kWave / 2; d > 0; d /= 2) value += __shfl_xor(value, d, kWave);
    if (lane == 0) sh[wave] = value;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += sh[w];
    return (int)total;
}

__global__ __launch_bounds__(kBlock) void classify_kernel(Volume vol, unsigned char* __restrict__ cell_code,
                                                          int* __restrict__ tri_counts, MeshDev p) {
    const long long sy = p.nx, sz = (long long)p.nx * p.ny;
    const long long tile = (long long)blockIdx.x * kTile;
    unsigned tris = 0;
    for (int r = 0; r < kSteps; ++r) {
        const long long v = tile + r * kBlock + threadIdx.x;
        if (v >= p.voxels) break;
        int k, j, i;
        coords(v, p, k, j, i);
        unsigned code = 0;
        if (k < p.nx - 1 && j < p.ny - 1 && i < p.nz - 1) {
            bool valid = true;
            unsigned c8 = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const long long q = v + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
                valid = valid && usable(vol, q, p);
                c8 |= ((double)vol.tsdf[q] < p.iso ? 1u : 0u) << c;
            }
            code = valid ? c8 : 0u;
        }
        cell_code[v] = (unsigned char)code;
        tris += kMeshTriangleCount[code];
    }
    const int total = block_sum(tris);
    if (threadIdx.x == 0) tri_counts[blockIdx.x] = total;
}

// whether cell (i, j, k) exists (>= 0 on every axis) and its code crosses the edge from corner c to c + d
__device__ inline unsigned crosses(const unsigned char* __restrict__ cell_code, long long v, bool exists, int c,
                                   int d) {
    if (!exists) return 0u;
    const unsigned code = cell_code[v];
    return ((code >> c) ^ (code >> (c + d))) & 1u;
}

__global__ __launch_bounds__(kBlock) void edges_kernel(const unsigned char* __restrict__ cell_code,
                                                       unsigned char* __restrict__ edge_mask,
                                                       int* __restrict__ vertex_counts, MeshDev p) {
    const long long sy = p.nx, sz = (long long)p.nx * p.ny;
    const long long tile = (long long)blockIdx.x * kTile;
    unsigned verts = 0;
    for (int r = 0; r < kSteps; ++r) {
        const long long v = tile + r * kBlock + threadIdx.x;
        if (v >= p.voxels) break;
        int k, j, i;
        coords(v, p, k, j, i);
        // the voxel is corner (x, y, z) of cell v - (x + y sy + z sz); cells on the high borders have code 0
        unsigned ex = 0, ey = 0, ez = 0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                ex |= crosses(cell_code, v - b * sy - a * sz, j >= b && i >= a, 2 * b + 4 * a, 1);  // corner (0, b, a)
                ey |= crosses(cell_code, v - b - a * sz, k >= b && i >= a, b + 4 * a, 2);        // corner (b, 0, a)
                ez |= crosses(cell_code, v - b - a * sy, k >= b && j >= a, b + 2 * a, 4);        // corner (b, a, 0)
            }
        const unsigned m = ex | (ey << 1) | (ez << 2);
        edge_mask[v] = (unsigned char)m;
        verts += (unsigned)__popc(m);
    }
    const int total = block_sum(verts);
    if (threadIdx.x == 0) vertex_counts[blockIdx.x] = total;
}

// one workgroup: each of the two count arrays becomes its exclusive prefix (in place, int32: the totals are bounded
// on the host) and its total goes to totals[]
__global__ __launch_bounds__(kScanThreads) void scan_kernel(int* __restrict__ offsets, long long* __restrict__ totals,
                                                            int blocks) {
    __shared__ long long sh[kScanThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (int arr = 0; arr < 2; ++arr) {
        int* a = offsets + (long long)arr * blocks;
        long long running = 0;
        for (int base = 0; base < blocks; base += kScanThreads) {
            const int idx = base + threadIdx.x;
            const long long x = idx < blocks ? a[idx] : 0;
            long long incl = x;
#pragma unroll
            for (int d = 1; d < kWave; d *= 2) {
                const long long y = __shfl_up(incl, d, kWave);
                if (lane >= d) incl += y;
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
        if (threadIdx.x == 0) totals[arr] = running;
    }
}

// the float64 gradient of the tsdf along axis at voxel v (index `at` of n on that axis, stride s)
__device__ inline double gradient(const Volume& vol, long long v, int at, int n, long long s, const MeshDev& p) {
    const bool up = at + 1 < n && usable(vol, v + s, p);
    const bool dn = at >= 1 && usable(vol, v - s, p);
    const double c = (double)vol.tsdf[v];
    if (up && dn) return ((double)vol.tsdf[v + s] - (double)vol.tsdf[v - s]) / 2.0;
    if (up) return (double)vol.tsdf[v + s] - c;
    if (dn) return c - (double)vol.tsdf[v - s];
    return 0.0;
}

__global__ __launch_bounds__(kBlock) void vertices_kernel(Volume vol, const unsigned char* __restrict__ edge_mask,
                                                          const int* __restrict__ offsets,
                                                          int* __restrict__ vertex_base, float* __restrict__ vertices,
                                                          float* __restrict__ normals, long long vertex_count,
                                                          MeshDev p) {
    __shared__ unsigned sh[2][kWaves];
    const long long sz = (long long)p.nx * p.ny;
    const long long stride[3] = {1, p.nx, sz};
    const int n[3] = {p.nx, p.ny, p.nz};
    const long long tile = (long long)blockIdx.x * kTile;
    long long next = offsets[blockIdx.x];
    for (int r = 0; r < kSteps; ++r) {  // every lane takes every step: block_scan holds a barrier
        const long long v = tile + r * kBlock + threadIdx.x;
        const unsigned m = v < p.voxels ? edge_mask[v] : 0u;
        unsigned prefix, total;
        block_scan<2>((unsigned)__popc(m), sh, r & 1, prefix, total);
        long long id = next + prefix;
        next += total;
        if (!m) continue;
        vertex_base[v] = (int)id;
        int g[3];  // (x, y, z)
        coords(v, p, g[0], g[1], g[2]);
        for (int axis = 0; axis < 3; ++axis) {
            if (!((m >> axis) & 1u) || id >= vertex_count) continue;
            const long long w = v + stride[axis];
            const double a = (double)vol.tsdf[v], b = (double)vol.tsdf[w];
            const double t = (p.iso - a) / (b - a);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double q = j == axis ? (double)g[j] + t : (double)g[j];
                vertices[id * 3 + j] = (float)((q + p.off[j]) * p.voxel);
            }
            if (normals) {
                double nv[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int gw = g[j] + (j == axis ? 1 : 0);
                    const double ga = gradient(vol, v, g[j], n[j], stride[j], p);
                    const double gb = gradient(vol, w, gw, n[j], stride[j], p);
                    nv[j] = ga * (1.0 - t) + gb * t;
                }
                const double len = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
#pragma unroll
                for (int j = 0; j < 3; ++j) normals[id * 3 + j] = len != 0.0 ? (float)(nv[j] / len) : 0.0f;
            }
            ++id;
        }
    }
}

__global__ __launch_bounds__(kBlock) void faces_kernel(const unsigned char* __restrict__ cell_code,
                                                       const unsigned char* __restrict__ edge_mask,
                                                       const int* __restrict__ offsets,
                                                       const int* __restrict__ vertex_base, int* __restrict__ faces,
                                                       long long face_count, MeshDev p) {
    __shared__ unsigned sh[2][kWaves];
    const long long sy = p.nx, sz = (long long)p.nx * p.ny;
    const long long tile = (long long)blockIdx.x * kTile;
    long long next = offsets[blockIdx.x];
    for (int r = 0; r < kSteps; ++r) {
        const long long v = tile + r * kBlock + threadIdx.x;
        const unsigned code = v < p.voxels ? cell_code[v] : 0u;
        const unsigned count = kMeshTriangleCount[code];
        unsigned prefix, total;
        block_scan<3>(count, sh, r & 1, prefix, total);
        const long long first = next + prefix;
        next += total;
        for (unsigned tri = 0; tri < count; ++tri) {
            const long long slot = first + tri;
            if (slot >= face_count) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = kMeshTriangleEdges[code][3 * tri + c];
                const int low = kMeshEdgeLow[e], axis = e / 4;
                const long long owner = v + (low & 1) + ((low >> 1) & 1) * sy + (low >> 2) * sz;
                const unsigned below = edge_mask[owner] & ((1u << axis) - 1u);
                faces[slot * 3 + c] = vertex_base[owner] + __popc(below);
            }
        }
    }
}

// one channel as a byte: floor(min(max(x, 0), 255) + 0.5), 0 for a NaN
__device__ inline unsigned char colour_byte(double x) {
    if (isnan(x)) return 0;
    const double lo = x > 0.0 ? x : 0.0;
    const double hi = lo < 255.0 ? lo : 255.0;
    return (unsigned char)floor(hi + 0.5);
}

struct DefaultColour {
    unsigned char c[3];
};

__global__ __launch_bounds__(kBlock) void vertex_colours_kernel(const float* __restrict__ tsdf,
                                                                const float4* __restrict__ colour,
                                                                const unsigned char* __restrict__ edge_mask,
                                                                const int* __restrict__ vertex_base,
                                                                unsigned char* __restrict__ colours,
                                                                long long vertex_count, DefaultColour fallback,
                                                                MeshDev p) {
    const long long stride[3] = {1, p.nx, (long long)p.nx * p.ny};
    const int n[3] = {p.nx, p.ny, p.nz};
    const long long tile = (long long)blockIdx.x * kTile;
    for (int r = 0; r < kSteps; ++r) {
        const long long v = tile + r * kBlock + threadIdx.x;
        if (v >= p.voxels) break;
        const unsigned m = edge_mask[v];
        if (!m) continue;
        long long id = vertex_base[v];
        int g[3];  // (x, y, z)
        coords(v, p, g[0], g[1], g[2]);
        const float4 ca = colour[v];
        for (int axis = 0; axis < 3; ++axis) {
            if (!((m >> axis) & 1u)) continue;
            if (id < 0 || id >= vertex_count || g[axis] + 1 >= n[axis]) break;  // not lsf_mesh_emit's workspaces
            const long long w = v + stride[axis];
            const double a = (double)tsdf[v], b = (double)tsdf[w];
            const double t = (p.iso - a) / (b - a);
            const float4 cb = colour[w];
            const bool has_a = ca.w > 0.0f, has_b = cb.w > 0.0f;  // NaN weights fail
            const float va[3] = {ca.x, ca.y, ca.z}, vb[3] = {cb.x, cb.y, cb.z};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                unsigned char out = fallback.c[j];
                if (has_a && has_b) out = colour_byte((double)va[j] * (1.0 - t) + (double)vb[j] * t);
                else if (has_a) out = colour_byte((double)va[j]);
                else if (has_b) out = colour_byte((double)vb[j]);
                colours[id * 3 + j] = out;
            }
            ++id;
        }
    }
}

bool finite(double x) { return std::isfinite(x); }

int convert(const lsf_mesh_params* q, MeshDev& p) {
    if (!q) return LSF_ERR_BAD_ARGUMENT;
    if (q->depth < 2 || q->height < 2 || q->width < 2) return LSF_ERR_BAD_ARGUMENT;
    const long long voxels = (long long)q->depth * q->height * q->width;
    const long long cells = (long long)(q->depth - 1) * (q->height - 1) * (q->width - 1);
    if (voxels > 0x7fffffffll / 3 || cells > 0x7fffffffll / LSF_MESH_MAX_TRIANGLES) return LSF_ERR_BAD_ARGUMENT;
    const double all[] = {q->voxel_size, q->offset_x, q->offset_y, q->offset_z, q->iso};
    for (double x : all)
        if (!finite(x)) return LSF_ERR_BAD_ARGUMENT;
    if (!(q->voxel_size > 0.0) || std::isnan(q->min_weight)) return LSF_ERR_BAD_ARGUMENT;
    p.voxel = q->voxel_size;
    p.iso = q->iso;
    p.min_weight = q->min_weight;
    p.off[0] = q->offset_x; p.off[1] = q->offset_y; p.off[2] = q->offset_z;
    p.nx = q->width; p.ny = q->height; p.nz = q->depth;
    p.voxels = voxels;
    p.blocks = (int)((voxels + kTile - 1) / kTile);
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

extern "C" int lsf_mesh_count(const float* tsdf, const float* weight, uint8_t* cell_code, uint8_t* edge_mask,
                              int32_t* block_offsets, int64_t* totals, const lsf_mesh_params* params, void* stream) {
    (void)hipGetLastError();
    if (!tsdf || !weight || !cell_code || !edge_mask || !block_offsets || !totals || tsdf == weight)
        return LSF_ERR_BAD_ARGUMENT;
    MeshDev p;
    if (int e = convert(params, p)) return e;
    const size_t n = (size_t)p.voxels;
    const void* const ins[2] = {tsdf, weight};
    const size_t in_bytes[2] = {n * 4, n * 4};
    const void* const outs[4] = {cell_code, edge_mask, block_offsets, totals};
    const size_t out_bytes[4] = {n, n, (size_t)p.blocks * 8, 16};
    if (any_alias(ins, in_bytes, outs, out_bytes)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const Volume vol{tsdf, weight};
    int* const vertex_counts = block_offsets;
    int* const tri_counts = block_offsets + p.blocks;
    hipLaunchKernelGGL(classify_kernel, dim3(p.blocks), dim3(kBlock), 0, s, vol, cell_code, tri_counts, p);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(edges_kernel, dim3(p.blocks), dim3(kBlock), 0, s, cell_code, edge_mask, vertex_counts, p);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_offsets,
                       reinterpret_cast<long long*>(totals), p.blocks);
    return launch_status();
}

extern "C" int lsf_mesh_emit(const float* tsdf, const float* weight, const uint8_t* cell_code, const uint8_t* edge_mask,
                             const int32_t* block_offsets, int32_t* vertex_base, float* vertices, float* normals,
                             int32_t* faces, int64_t vertex_count, int64_t face_count, const lsf_mesh_params* params,
                             void* stream) {
    (void)hipGetLastError();
    MeshDev p;
    if (int e = convert(params, p)) return e;
    if (!tsdf || !weight || !cell_code || !edge_mask || !block_offsets || tsdf == weight) return LSF_ERR_BAD_ARGUMENT;
    if (vertex_count < 0 || face_count < 0 || vertex_count > 3 * p.voxels ||
        face_count > (long long)LSF_MESH_MAX_TRIANGLES * (p.nx - 1) * (p.ny - 1) * (p.nz - 1))
        return LSF_ERR_BAD_ARGUMENT;
    if (vertex_count == 0 && face_count == 0) return 0;
    if (vertex_count == 0 || !vertex_base || !vertices || !faces) return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.voxels, vb = (size_t)vertex_count * 12;
    const void* const ins[5] = {tsdf, weight, cell_code, edge_mask, block_offsets};
    const size_t in_bytes[5] = {n * 4, n * 4, n, n, (size_t)p.blocks * 8};
    const void* const outs[4] = {vertex_base, vertices, normals, faces};
    const size_t out_bytes[4] = {n * 4, vb, vb, (size_t)face_count * 12};
    if (any_alias(ins, in_bytes, outs, out_bytes)) return LSF_ERR_BAD_ARGUMENT;
    hipStream_t s = as_stream(stream);
    const Volume vol{tsdf, weight};
    hipLaunchKernelGGL(vertices_kernel, dim3(p.blocks), dim3(kBlock), 0, s, vol, edge_mask, block_offsets, vertex_base,
                       vertices, normals, (long long)vertex_count, p);
    if (int e = launch_status()) return e;
    if (face_count == 0) return 0;
    hipLaunchKernelGGL(faces_kernel, dim3(p.blocks), dim3(kBlock), 0, s, cell_code, edge_mask, block_offsets + p.blocks,
                       vertex_base, faces, (long long)face_count, p);
    return launch_status();
}

extern "C" int lsf_mesh_vertex_colours(const float* tsdf, const float* colour, const uint8_t* edge_mask,
                                       const int32_t* vertex_base, uint8_t* colours, int64_t vertex_count,
                                       int32_t default_red, int32_t default_green, int32_t default_blue,
                                       const lsf_mesh_params* params, void* stream) {
    (void)hipGetLastError();
    MeshDev p;
    if (int e = convert(params, p)) return e;
    if (vertex_count < 0 || vertex_count > 3 * p.voxels) return LSF_ERR_BAD_ARGUMENT;
    const int32_t rgb[3] = {default_red, default_green, default_blue};
    DefaultColour fallback;
    for (int j = 0; j < 3; ++j) {
        if (rgb[j] < 0 || rgb[j] > 255) return LSF_ERR_BAD_ARGUMENT;
        fallback.c[j] = (unsigned char)rgb[j];
    }
    if (vertex_count == 0) return 0;
    if (!tsdf || !colour || !edge_mask || !vertex_base || !colours) return LSF_ERR_BAD_ARGUMENT;
    if (((uintptr_t)colour & 15) != 0) return LSF_ERR_BAD_ARGUMENT;
    const size_t n = (size_t)p.voxels;
    const void* const ins[4] = {tsdf, colour, edge_mask, vertex_base};
    const size_t in_bytes[4] = {n * 4, n * 16, n, n * 4};
    const void* const outs[1] = {colours};
    const size_t out_bytes[1] = {(size_t)vertex_count * 3};
    if (any_alias(ins, in_bytes, outs, out_bytes)) return LSF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(vertex_colours_kernel, dim3(p.blocks), dim3(kBlock), 0, as_stream(stream), tsdf,
                       reinterpret_cast<const float4*>(colour), edge_mask, vertex_base, colours, (long long)vertex_count,
                       fallback, p);
    return launch_status();
}
