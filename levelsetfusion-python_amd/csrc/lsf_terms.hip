// One term of the Slavcheva-style energy on its own (lsf_term_gradient, include/lsf_hip.h): the term-level functions of
// nonrigid_opt/slavcheva/{data_term,smoothing_term,level_set_term}.py.  One thread per selected voxel (grid-stride, x
// fastest), one kernel per (D, term): every term is its own code path.  The arithmetic is that of the fused kernels
// (lsf_slavcheva_terms.h, whose helpers the smoothing terms call) in the operation order of oracle/lsf_oracle.py;
// -ffp-contract=off keeps multiply and add separately rounded.
#include "lsf_slavcheva_terms.h"

namespace lsf {
namespace {

constexpr int kTermBlock = 256;
constexpr unsigned kTermMaxBlocks = 2048;  // 8 waves per CU on 256 CUs; grid-stride beyond, and at most 2048 atomics

// one component of a vector field: base of component c, stride between voxels (1 planar, D interleaved)
struct TField {
    const float* p;
    long long cs;
};

// Neighbourhood of one voxel with the interface of slav::Nbh (killing_gradient calls it): clamped neighbour offsets,
// `has` says whether a neighbour exists.  With copy_if_zero (2-D only) a diagonal neighbour whose warp vector has norm 0
// counts as missing, so that killing_gradient reads the centre value for it as for one outside the array.
template <int D>
struct TermNbh {
    using Field = TField;
    long long i;
    int off[3][2];
    bool has[3][2];
    bool zero_diag[2][2];  // (x, y) diagonal [sx][sy] has norm 0 (copy_if_zero)

    __device__ inline TermNbh(const Grid& g, int x, int y, int z, long long v) : i(v) {
        const int stride[3] = {1, g.nx, g.nx * g.ny};
        const int coord[3] = {x, y, z};
        const int extent[3] = {g.nx, g.ny, g.nz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            has[a][0] = a < D && coord[a] > 0;
            has[a][1] = a < D && coord[a] < extent[a] - 1;
            off[a][0] = has[a][0] ? -stride[a] : 0;
            off[a][1] = has[a][1] ? stride[a] : 0;
        }
        zero_diag[0][0] = zero_diag[0][1] = zero_diag[1][0] = zero_diag[1][1] = false;
    }
    __device__ inline bool exists(int a, int s) const { return has[a][s]; }
    __device__ inline float at(const Field& f, long long o) const { return f.p[(i + o) * f.cs]; }
    __device__ inline float centre(const Field& f) const { return at(f, 0); }
    __device__ inline float axis(const Field& f, int a, int s) const { return at(f, off[a][s]); }
    __device__ inline float diag(const Field& f, int a, int sa, int b, int sb) const {
        return at(f, off[a][sa] + off[b][sb]);
    }
    __device__ inline bool diag_exists(int a, int sa, int b, int sb) const {
        return has[a][sa] && has[b][sb] && !(D == 2 && zero_diag[sa][sb]);
    }
};

// utils/sampling.py:91-96: np.linalg.norm(w) == 0.0, the float32 norm of the float32 vector
__device__ inline bool norm_is_zero(float u, float v) { return u * u + v * v == 0.0f; }

struct TermArgs {
    const float *live, *canonical, *lg[3];
    TField warp[3];
    float* g_out;
    long long g_cs, g_ps;  // output strides: between entries, between components
    double *e_out, *e_total;
    const int* indices;
    long long count;
    slav::Params sp;
    float epsilon, scaling;
    int copy_if_zero, ignore_if_zero, select, np_gradient_energy;
};

// level_set_term.py:28-64 (OOB -> 1; second derivatives use the +1 neighbour twice, level_set_term.py:47-48): the
// arithmetic of slav::level_set_gradient and oracle.level_set_gradient, with epsilon a parameter
template <int D>
__device__ inline void level_set_term(const TermNbh<D>& n, const TField& live, float eps, float (&gl)[3], float& energy) {
    const float l = n.centre(live);
    float grad[3] = {0.0f, 0.0f, 0.0f};
    float hess[3][3];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float lp = n.exists(c, 1) ? n.axis(live, c, 1) : 1.0f;
        const float lm = n.exists(c, 0) ? n.axis(live, c, 0) : 1.0f;
        grad[c] = (0.5f * (lp - lm)) * 10.0f;
        hess[c][c] = ((lp - 2.0f * l) + lp) * 10.0f;
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a + 1; b < D; ++b) {
            const float pp = n.diag_exists(a, 1, b, 1) ? n.diag(live, a, 1, b, 1) : 1.0f;
            const float mp = n.diag_exists(a, 0, b, 1) ? n.diag(live, a, 0, b, 1) : 1.0f;
            const float pm = n.diag_exists(a, 1, b, 0) ? n.diag(live, a, 1, b, 0) : 1.0f;
            const float mm = n.diag_exists(a, 0, b, 0) ? n.diag(live, a, 0, b, 0) : 1.0f;
            const float s = (a == 0 && b == 1) ? ((pp - mp) - pm) + mm   // level_set_term.py:52-53
                                               : ((pp - pm) - mp) + mm;  // pairs with z: z difference first
            const float h = (0.25f * s) * 10.0f;
            hess[a][b] = h;
            hess[b][a] = h;
        }
    float sq = grad[0] * grad[0];
#pragma unroll
    for (int c = 1; c < D; ++c) sq = sq + grad[c] * grad[c];
    const float nrm = sqrtf(sq);
    const float coef = (1.0f - nrm) / (nrm + eps);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        float hv = hess[i][0] * grad[0];
#pragma unroll
        for (int j = 1; j < D; ++j) hv = hv + hess[i][j] * grad[j];
        gl[i] = coef * hv;
    }
    const float dn = nrm - 1.0f;
    energy = 0.5f * (dn * dn);
}

// gradient and local energy of term TERM at voxel v
template <int D, int TERM>
__device__ inline void term_at(const TermArgs& A, const Grid& g, int x, int y, int z, long long v, float (&gv)[3],
                               float& e) {
    TermNbh<D> n(g, x, y, z, v);
    if (TERM == LSF_TERM_DATA_BASIC || TERM == LSF_TERM_DATA_THRESHOLDED_FDM) {
        const float l = A.live[v];
        const float diff = l - A.canonical[v];
        if (A.g_out) {
            const TField live{A.live, 1};
#pragma unroll
            for (int a = 0; a < D; ++a) {
                float lg = A.lg[a][v];  // the caller's gradient
                if (TERM == LSF_TERM_DATA_THRESHOLDED_FDM) {
                    // data_term.py:203-210: above 0.5 take the smaller one-sided difference (the backward one on a
                    // tie), and 0 if that too is above 0.5; neighbours outside the array read 1
                    const float fwd = (n.exists(a, 1) ? n.axis(live, a, 1) : 1.0f) - l;
                    const float bwd = l - (n.exists(a, 0) ? n.axis(live, a, 0) : 1.0f);
                    float alt = fabsf(fwd) < fabsf(bwd) ? fwd : bwd;
                    alt = fabsf(alt) > 0.5f ? 0.0f : alt;
                    lg = fabsf(lg) > 0.5f ? alt : lg;
                }
                gv[a] = (diff * lg) * A.scaling;
            }
        }
        e = 0.5f * (diff * diff);  // data_term.py:185
        return;
    }
    if (TERM == LSF_TERM_LEVEL_SET) {
        level_set_term<D>(n, TField{A.live, 1}, A.epsilon, gv, e);
        return;
    }
    // ---- smoothing terms
    const TField(&w)[3] = A.warp;
    float wc[3] = {0.0f, 0.0f, 0.0f}, wm[3][3], wp[3][3];  // wm/wp[a][c]: clamped (missing -> centre)
#pragma unroll
    for (int c = 0; c < D; ++c) {
        wc[c] = n.centre(w[c]);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            wm[a][c] = n.axis(w[c], a, 0);
            wp[a][c] = n.axis(w[c], a, 1);
        }
    }
    if (D == 2 && TERM == LSF_TERM_TIKHONOV_LOCAL && A.ignore_if_zero) {
        // smoothing_term.py:108-113: np.linalg.norm(w == 0.0) is the norm of a BOOLEAN vector -- non-zero as soon as
        // one component of an existing 4-neighbour is 0
        bool any = false;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                any = any || (n.exists(a, 0) && wm[a][c] == 0.0f) || (n.exists(a, 1) && wp[a][c] == 0.0f);
        if (any) {
            gv[0] = gv[1] = 0.0f;
            e = 0.0f;
            return;
        }
    }
    // neighbours as the gradient reads them: copy_if_zero also replaces those of norm 0 with the centre
    float um[3][3], up[3][3];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            um[a][c] = wm[a][c];
            up[a][c] = wp[a][c];
        }
    if (D == 2 && A.copy_if_zero) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (norm_is_zero(wm[a][0], wm[a][1])) um[a][0] = wc[0], um[a][1] = wc[1];
            if (norm_is_zero(wp[a][0], wp[a][1])) up[a][0] = wc[0], up[a][1] = wc[1];
        }
        if (TERM == LSF_TERM_KILLING) {
#pragma unroll
            for (int sx = 0; sx < 2; ++sx)
#pragma unroll
                for (int sy = 0; sy < 2; ++sy)
                    n.zero_diag[sx][sy] = norm_is_zero(n.diag(w[0], 0, sx, 1, sy), n.diag(w[1], 0, sx, 1, sy));
        }
    }
    if (TERM == LSF_TERM_KILLING) {
        double ek = 0.0;
        slav::killing_gradient<D, TermNbh<D>>(n, w, um, up, wc, A.sp, gv, ek, A.e_out || A.e_total);
        e = (float)ek;  // the float32 local value, widened by the helper
        return;
    }
    if (TERM == LSF_TERM_TIKHONOV) {
        slav::tikhonov_gradient<D>(um, up, wc, gv);  // -scipy.ndimage.laplace, edge replicated
    } else {
        // smoothing_term.py:131-132: -(w[x+1] + w[y+1] - 4 w + w[x-1] + w[y-1]) in that order (3-D: z after y, 6 w)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            float s = up[0][c];
#pragma unroll
            for (int a = 1; a < D; ++a) s = s + up[a][c];
            s = s - (2.0f * D) * wc[c];
#pragma unroll
            for (int a = 0; a < D; ++a) s = s + um[a][c];
            gv[c] = -s;
        }
    }
    float es = 0.0f;
    if (A.np_gradient_energy) {
        // smoothing_term.py:168-176: np.gradient of every component, oracle.smoothing_energy_vectorized's order
#pragma unroll
        for (int c = 0; c < D; ++c)
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const float d = slav::np_gradient_from(n, a, wm[a][c], wp[a][c]);
                es = (a + c == 0) ? d * d : es + d * d;
            }
    } else {
        // smoothing_term.py:134-139 on the neighbours the gradient read, oracle.tikhonov_energy_direct's order
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const float der = 0.5f * (up[a][c] - um[a][c]);
                es = (a + c == 0) ? der * der : es + der * der;
            }
    }
    e = 0.5f * es;
}

template <int D, int TERM>
__global__ void __launch_bounds__(kTermBlock) term_kernel(TermArgs A, Grid g) {
    const long long n_total = (long long)g.nz * g.ny * g.nx;
    const long long step = (long long)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < A.count; k += step) {
        const long long v = A.select == LSF_SELECT_LIST ? (long long)A.indices[k] : k;
        float gv[3] = {0.0f, 0.0f, 0.0f};
        float e = 0.0f;
        bool active = v >= 0 && v < n_total;
        if (active && A.select == LSF_SELECT_BAND)
            active = !(fabsf(A.live[v]) == 1.0f && fabsf(A.canonical[v]) == 1.0f);
        if (active) {
            const unsigned row = fast_div((unsigned)v, g.div_nx);
            const int x = (int)((unsigned)v - row * (unsigned)g.nx);
            const int z = D == 3 ? (int)fast_div(row, g.div_ny) : 0;
            const int y = (int)(row - (unsigned)z * (unsigned)g.ny);
            term_at<D, TERM>(A, g, x, y, z, v, gv, e);
        }
        if (A.g_out) {
#pragma unroll
            for (int c = 0; c < D; ++c) A.g_out[k * A.g_cs + c * A.g_ps] = gv[c];
        }
        if (A.e_out) A.e_out[k] = (double)e;
        acc += (double)e;
    }
    if (A.e_total) {
        const double sums[1] = {acc};
        double* const dst[1] = {A.e_total};
        block_reduce_commit<1>(0ull, sums, nullptr, dst);
    }
}

template <int D, int TERM>
void launch(const TermArgs& A, const Grid& g, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((term_kernel<D, TERM>), dim3(blocks), dim3(kTermBlock), 0, s, A, g);
}

template <int D>
void launch_term(int term, const TermArgs& A, const Grid& g, unsigned blocks, hipStream_t s) {
    switch (term) {
        case LSF_TERM_DATA_BASIC: launch<D, LSF_TERM_DATA_BASIC>(A, g, blocks, s); break;
        case LSF_TERM_DATA_THRESHOLDED_FDM: launch<D, LSF_TERM_DATA_THRESHOLDED_FDM>(A, g, blocks, s); break;
        case LSF_TERM_TIKHONOV: launch<D, LSF_TERM_TIKHONOV>(A, g, blocks, s); break;
        case LSF_TERM_TIKHONOV_LOCAL: launch<D, LSF_TERM_TIKHONOV_LOCAL>(A, g, blocks, s); break;
        case LSF_TERM_KILLING: launch<D, LSF_TERM_KILLING>(A, g, blocks, s); break;
        default: launch<D, LSF_TERM_LEVEL_SET>(A, g, blocks, s); break;
    }
}

}  // namespace
}  // namespace lsf

using namespace lsf;

extern "C" int lsf_term_gradient(const float* live, const float* canonical, const float* live_gradient_x,
                                 const float* live_gradient_y, const float* live_gradient_z, const float* warp,
                                 float* gradient_out, double* energy_out, double* energy_total, const lsf_grid* grid,
                                 const lsf_term_params* params, int32_t selection, int32_t energy_form,
                                 const int32_t* indices, int64_t index_count, void* stream) {
    if (int e = check_grid(grid)) return e;
    if (!params || grid->z_begin != 0 || grid->z_end != grid->nz) return LSF_ERR_BAD_ARGUMENT;
    const int D = grid->dims, term = params->term, flags = params->flags;
    if (term < LSF_TERM_DATA_BASIC || term > LSF_TERM_LEVEL_SET) return LSF_ERR_BAD_ARGUMENT;
    if (flags & ~(LSF_TERM_COPY_IF_ZERO | LSF_TERM_IGNORE_IF_ZERO | LSF_TERM_INTERLEAVED)) return LSF_ERR_BAD_ARGUMENT;
    const bool data = term == LSF_TERM_DATA_BASIC || term == LSF_TERM_DATA_THRESHOLDED_FDM;
    const bool smoothing = term >= LSF_TERM_TIKHONOV && term <= LSF_TERM_KILLING;
    // copy_if_zero / ignore_if_zero: 2-D reference semantics only, and only the per-location smoothing terms have them
    if (flags & (LSF_TERM_COPY_IF_ZERO | LSF_TERM_IGNORE_IF_ZERO)) {
        if (D != 2 || (term != LSF_TERM_TIKHONOV_LOCAL && term != LSF_TERM_KILLING)) return LSF_ERR_BAD_ARGUMENT;
    }
    if (energy_form != LSF_TERM_ENERGY_LOCAL && energy_form != LSF_TERM_ENERGY_NP_GRADIENT) return LSF_ERR_BAD_ARGUMENT;
    if (energy_form == LSF_TERM_ENERGY_NP_GRADIENT && term != LSF_TERM_TIKHONOV && term != LSF_TERM_TIKHONOV_LOCAL)
        return LSF_ERR_BAD_ARGUMENT;
    if (selection != LSF_SELECT_ALL && selection != LSF_SELECT_BAND && selection != LSF_SELECT_LIST)
        return LSF_ERR_BAD_ARGUMENT;
    if (index_count < 0 || (selection == LSF_SELECT_LIST && index_count > 0 && !indices)) return LSF_ERR_BAD_ARGUMENT;
    if ((data || selection == LSF_SELECT_BAND) && (!live || !canonical)) return LSF_ERR_BAD_ARGUMENT;
    if (term == LSF_TERM_LEVEL_SET && !live) return LSF_ERR_BAD_ARGUMENT;
    if (smoothing && !warp) return LSF_ERR_BAD_ARGUMENT;
    if (data && gradient_out && (!live_gradient_x || !live_gradient_y || (D == 3 && !live_gradient_z)))
        return LSF_ERR_BAD_ARGUMENT;

    const long long n = (long long)grid->nz * grid->ny * grid->nx;
    const long long count = selection == LSF_SELECT_LIST ? (long long)index_count : n;
    if (count == 0 || (!gradient_out && !energy_out && !energy_total)) return 0;
    if (count > 0x7fffffffll) return LSF_ERR_BAD_DIMS;

    const bool interleaved = (flags & LSF_TERM_INTERLEAVED) != 0;
    TermArgs A;
    A.live = live;
    A.canonical = canonical;
    A.lg[0] = live_gradient_x;
    A.lg[1] = live_gradient_y;
    A.lg[2] = live_gradient_z;
    for (int c = 0; c < 3; ++c) {
        const int cc = c < D ? c : 0;
        A.warp[c] = TField{warp ? warp + (interleaved ? cc : cc * n) : nullptr, interleaved ? (long long)D : 1ll};
    }
    A.g_out = gradient_out;
    A.g_cs = interleaved ? D : 1;
    A.g_ps = interleaved ? 1 : count;
    A.e_out = energy_out;
    A.e_total = energy_total;
    A.indices = indices;
    A.count = count;
    A.sp.lambda64 = params->isomorphic_enforcement_factor_f64;
    A.sp.lambda32 = params->isomorphic_enforcement_factor;
    A.sp.killing_c1 = (float)(-2.0 * (1.0 + params->isomorphic_enforcement_factor_f64));  // smoothing_term.py:90
    A.sp.rate = A.sp.w_data = A.sp.w_smooth = A.sp.w_level_set = 0.0f;
    A.sp.zero_gradient_on_snap = 0;
    A.epsilon = params->epsilon;
    A.scaling = params->scaling_factor;
    A.copy_if_zero = (flags & LSF_TERM_COPY_IF_ZERO) != 0;
    A.ignore_if_zero = term == LSF_TERM_TIKHONOV_LOCAL && (flags & LSF_TERM_IGNORE_IF_ZERO) != 0;
    A.select = selection;
    A.np_gradient_energy = energy_form == LSF_TERM_ENERGY_NP_GRADIENT;

    const Grid g = make_grid(grid);
    const unsigned long long want = (unsigned long long)((count + kTermBlock - 1) / kTermBlock);
    const unsigned blocks = (unsigned)(want < kTermMaxBlocks ? want : kTermMaxBlocks);
    if (D == 2)
        launch_term<2>(term, A, g, blocks, as_stream(stream));
    else
        launch_term<3>(term, A, g, blocks, as_stream(stream));
    return launch_status();
}
