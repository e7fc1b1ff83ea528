// The solve of the SDF-2-SDF rigid trackers, templated on the twist size N (lsf_rigid.hip: N = 3, lsf_rigid3d.hip:
// N = 6): the layouts of the per-block partial sums and of the per-iteration record, the fixed-order reductions of
// the partials, the N x N inverse, and the kernel prologue that turns iteration k-1's partials into the twist of
// launch k.  Each tracker keeps its own per-voxel body; everything from the partial sums on is decided here once.
// Projective ICP (lsf_icp.hip) shares the reductions, the normal equations' layout and the solve; its update (a
// composition, not the SDF-2-SDF blend) and its record are its own.
// The partials cross a launch boundary only (cdna_hip_programming.md, split-K item 2, the launch-boundary reduce): no
// atomics, no in-launch hand-off, and the reductions add in one fixed order, so a run is bit-reproducible.
// The prologue and the update are forced inline: a template of a header has vague linkage and is otherwise kept out
// of line, and the call would cost the kernels VGPRs and scratch that the inlined code does not.
#pragma once

#include "lsf_device.h"

namespace lsf {

enum RigidMode {
    GRADIENT = 0,  // the twist gradient of one live field (one launch)
    ITERATE = 1,   // iteration k: prologue (combine k-1, update, record k-1), then the body's partial sums
    FINISH = 2     // the prologue alone for the last iteration, one block; writes the final twist
};

// partial sums: A's upper triangle row by row, then b, then the energy sum.
// record: [twist* (N)][twist (N)][energy][A (N x N)][b (N)][skipped][zeros up to kRecord]
template <int N>
struct RigidLayout {
    static_assert(N == 3 || N == 6, "the 2-D and the 6-DoF tracker");
    static constexpr int kSums = N * (N + 1) / 2 + N + 1;
    static constexpr int kTwistStar = 0, kTwist = N, kEnergy = 2 * N, kA = 2 * N + 1, kB = kA + N * N,
                         kSkipped = kB + N;
    static constexpr int kRecord = N == 3 ? LSF_RIGID_RECORD_DOUBLES : LSF_RIGID3D_RECORD_DOUBLES;
    static constexpr int kMaxBlocks = N == 3 ? LSF_RIGID_MAX_BLOCKS : LSF_RIGID3D_MAX_BLOCKS;
    static constexpr int kScratchBytes = N == 3 ? LSF_RIGID_SCRATCH_BYTES : LSF_RIGID3D_SCRATCH_BYTES;
    static_assert(kSkipped < kRecord, "the record holds every field");
    static_assert(kScratchBytes == 2 * kMaxBlocks * kSums * 8, "two ping-pong buffers of kMaxBlocks partials");
    static_assert(kMaxBlocks <= kBlock, "the prologue gives every partial one thread");
};

// butterfly sum over the wave; every lane ends with the total.  Not wave_sum_f64 (DPP): that one adds in another
// order, and the records are pinned to this one's bits
__device__ inline double wave_sum_xor(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of v[] over the block in a fixed order; the totals land in thread 0's v[]
template <int K>
__device__ inline void block_sum(double (&v)[K], double (*red)[K]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = wave_sum_xor(v[c]);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) red[wave][c] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double s = red[0][c];
            for (int q = 1; q < kBlock / kWave; ++q) s += red[q][c];
            v[c] = s;
        }
    __syncthreads();
}

// N x N inverse by LU with partial pivoting (LAPACK getrf/getri's pivot rule: first largest magnitude); false on an
// exact zero pivot -- A == 0, a zero row and column (a twist-gradient component that is 0 at every voxel), or any other
// A the elimination finds exactly singular: the cases where the reference's np.linalg.cond(A) is inf and it skips the
// update
template <int N>
__device__ inline bool invert(const double a[N * N], double inv[N * N]) {
    double m[N][N];
    int perm[N];
    for (int i = 0; i < N; ++i) {
        perm[i] = i;
        for (int j = 0; j < N; ++j) m[i][j] = a[i * N + j];
    }
    for (int c = 0; c < N; ++c) {
        int piv = c;
        for (int r = c + 1; r < N; ++r)
            if (fabs(m[r][c]) > fabs(m[piv][c])) piv = r;
        if (m[piv][c] == 0.0) return false;
        if (piv != c) {
            for (int j = 0; j < N; ++j) { const double t = m[c][j]; m[c][j] = m[piv][j]; m[piv][j] = t; }
            const int t = perm[c]; perm[c] = perm[piv]; perm[piv] = t;
        }
        for (int r = c + 1; r < N; ++r) {
            m[r][c] = m[r][c] / m[c][c];
            for (int j = c + 1; j < N; ++j) m[r][j] = m[r][j] - m[r][c] * m[c][j];
        }
    }
    for (int col = 0; col < N; ++col) {  // solve L U x = P e_col
        double y[N];
        for (int i = 0; i < N; ++i) {
            double s = perm[i] == col ? 1.0 : 0.0;
            for (int j = 0; j < i; ++j) s = s - m[i][j] * y[j];
            y[i] = s;
        }
        for (int i = N - 1; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < N; ++j) s = s - m[i][j] * inv[j * N + col];
            inv[i * N + col] = s / m[i][i];
        }
    }
    return true;
}

// the fixed-order sum of nblocks partials of K sums each, part[block * K + c]: one partial per thread, then block_sum;
// the totals land in thread 0's v[]
template <int K>
__device__ __forceinline__ void combine_partials(const double* __restrict__ part, int nblocks, double (&v)[K],
                                                 double (*red)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = 0.0;
    if ((int)threadIdx.x < nblocks)
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = part[threadIdx.x * K + c];
    block_sum(v, red);
}

// the normal equations from their sums: A (N x N, row-major) from its upper triangle stored row by row at v[0], b (N)
// after it
template <int N>
__device__ __forceinline__ void normal_equations(const double* v, double a[N * N], double b[N]) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const int r = i < j ? i : j, c = i < j ? j : i;  // the upper triangle's entry
            a[i * N + j] = v[r * N - r * (r - 1) / 2 + (c - r)];
        }
    for (int i = 0; i < N; ++i) b[i] = v[N * (N + 1) / 2 + i];
}

// x = A^-1 b (x[i] = inv[i][0] b[0] + inv[i][1] b[1] + ..., left to right); 1 and x untouched when A holds a non-finite
// entry or invert<N> meets an exact zero pivot (the update is skipped), else 0
template <int N>
__device__ __forceinline__ int solve(const double a[N * N], const double b[N], double x[N]) {
    bool finite = true;
    for (int i = 0; i < N * N; ++i) finite = finite && isfinite(a[i]);
    double inv[N * N];
    if (!(finite && invert<N>(a, inv))) return 1;
    for (int i = 0; i < N; ++i) {
        double s = inv[i * N] * b[0];
        for (int j = 1; j < N; ++j) s = s + inv[i * N + j] * b[j];
        x[i] = s;
    }
    return 0;
}

// this block's K sums: reduced over the block (block_sum), thread 0 writes them to part[blockIdx.x * K + c]
template <int K>
__device__ __forceinline__ void store_partial(double (&acc)[K], double (*red)[K], double* __restrict__ part) {
    block_sum(acc, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) part[(size_t)blockIdx.x * K + c] = acc[c];
}

// combine iteration k-1 (partials in scratch buffer (k-1) & 1, twist before it in `prev`), singular test, update
// twist += rate (A^-1 b - twist), write record k-1 (block 0); the new twist goes to tw_out (LDS) for every thread
template <int N>
__device__ __forceinline__ void rigid_update(int k, int nblocks, double rate, const double* __restrict__ prev,
                                             double* __restrict__ records, const double* __restrict__ scratch,
                                             double (*red)[RigidLayout<N>::kSums], double* tw_out,
                                             double* twist_final) {
    using L = RigidLayout<N>;
    double v[L::kSums];
    const double* part = scratch + (size_t)((k - 1) & 1) * L::kMaxBlocks * L::kSums;
#pragma unroll
    for (int c = 0; c < L::kSums; ++c) v[c] = 0.0;
    if ((int)threadIdx.x < nblocks)
#pragma unroll
        for (int c = 0; c < L::kSums; ++c) v[c] = part[threadIdx.x * L::kSums + c];
    block_sum(v, red);
    if (threadIdx.x == 0) {
        double a[N * N], b[N];
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                const int r = i < j ? i : j, c = i < j ? j : i;  // the upper triangle's entry
                a[i * N + j] = v[r * N - r * (r - 1) / 2 + (c - r)];
            }
        for (int i = 0; i < N; ++i) b[i] = v[N * (N + 1) / 2 + i];
        const double energy = 0.5 * v[L::kSums - 1];
        double tw[N], ts[N];
        for (int i = 0; i < N; ++i) { tw[i] = prev[i]; ts[i] = 0.0; }
        bool finite = true;
        for (int i = 0; i < N * N; ++i) finite = finite && isfinite(a[i]);
        double inv[N * N];
        const int skipped = finite && invert<N>(a, inv) ? 0 : 1;
        if (skipped == 0) {
            for (int i = 0; i < N; ++i) {
                double s = inv[i * N] * b[0];
                for (int j = 1; j < N; ++j) s = s + inv[i * N + j] * b[j];
                ts[i] = s;
            }
            for (int i = 0; i < N; ++i) tw[i] = tw[i] + rate * (ts[i] - tw[i]);
        }
        for (int i = 0; i < N; ++i) tw_out[i] = tw[i];
        if (blockIdx.x == 0) {
            double* r = records + (size_t)(k - 1) * L::kRecord;
            for (int i = 0; i < N; ++i) { r[L::kTwistStar + i] = ts[i]; r[L::kTwist + i] = tw[i]; r[L::kB + i] = b[i]; }
            r[L::kEnergy] = energy;
            for (int i = 0; i < N * N; ++i) r[L::kA + i] = a[i];
            r[L::kSkipped] = (double)skipped;
            for (int i = L::kSkipped + 1; i < L::kRecord; ++i) r[i] = 0.0;
            if (twist_final)
                for (int i = 0; i < N; ++i) twist_final[i] = tw[i];
        }
    }
    __syncthreads();
}

// the twist of this launch into tw (LDS): p.twist (GRADIENT), twist_io (iteration 0), or iteration k-1 combined and
// applied to the twist before it -- record k-2's, or the initial one.  The finishing launch has one block, which reads
// twist_io before it writes it.  p: the tracker's launch parameters (twist, rate, nblocks).  The caller synchronises
// before it reads tw.
template <int MODE, int N, typename P>
__device__ __forceinline__ void rigid_prologue(const P& p, int k, double* __restrict__ twist_io,
                                               double* __restrict__ records, const double* __restrict__ scratch,
                                               double (*red)[RigidLayout<N>::kSums], double* tw) {
    if (MODE == GRADIENT) {
        if (threadIdx.x == 0)
            for (int i = 0; i < N; ++i) tw[i] = p.twist[i];
    } else if (k == 0) {
        if (threadIdx.x == 0)
            for (int i = 0; i < N; ++i) tw[i] = twist_io[i];
    } else {
        using L = RigidLayout<N>;
        const double* prev = k >= 2 ? records + (size_t)(k - 2) * L::kRecord + L::kTwist : twist_io;
        rigid_update<N>(k, p.nblocks, p.rate, prev, records, scratch, red, tw, MODE == FINISH ? twist_io : nullptr);
    }
}

// this block's partial sums of iteration k into scratch buffer k & 1
template <int N>
__device__ inline void rigid_store_partial(double (&acc)[RigidLayout<N>::kSums], double (*red)[RigidLayout<N>::kSums],
                                           double* __restrict__ scratch, int k) {
    using L = RigidLayout<N>;
    block_sum(acc, red);
    if (threadIdx.x == 0) {
        double* part = scratch + (size_t)(k & 1) * L::kMaxBlocks * L::kSums + (size_t)blockIdx.x * L::kSums;
#pragma unroll
        for (int c = 0; c < L::kSums; ++c) part[c] = acc[c];
    }
}

}  // namespace lsf
