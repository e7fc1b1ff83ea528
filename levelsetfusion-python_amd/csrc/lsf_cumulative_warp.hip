// The cumulative warp of a KillingFusion call ("Cumulative warp"), D = 2, 3.
//
// Every iteration of the Slavcheva-style optimizer re-warps the live field by its own update u_k:
// live_{k+1}(v) = live_k(v + u_k(v)) (slavcheva_optimizer2d.py:324-328), so the displacements compose,
//     PSI_0 = 0,   PSI_{k+1}(v) = u_k(v) + PSI_k(v + u_k(v)),          live_0(v + PSI(v)) ~ canonical(v),
// and PSI is what lsf_fusion_integrate_depth_warped takes.  The rule, per voxel and component c, with u the update the
// state holds BEHIND the iteration (zeroed where the re-warped live value snapped to +-1, field_warping.py:138-141):
//     PSI'_c(v) = float32( u_c(v) + S_c ),   S_c = sample_linear(PSI_c, position(v, u), oob = 0)
// position = float32(coordinate) + u per axis in float32 (the oracle's _grid_positions), sample_linear the oracle's: lerp z,
// then y, then x, every tap outside the array reads 0, multiply and add rounded separately.  Outside the band u = 0 and
// PSI stays 0: only listed voxels are visited, everything else of BOTH ping-pong buffers holds zeros for ever.
//
// PSI layout: float4 [z][y][x] = (unused, x, y, z), the state's channel order -- a tap is one 16-byte load (DESIGN.md
// section 4), and lsf_state_unpack turns the final buffer into the API layout.  Per listed voxel and iteration the
// compulsory traffic is 16 B (state) + 16 B (PSI in, the voxel's own cell) + 16 B (PSI out); the other 2^D - 1 taps are
// neighbours' cells.  One launch, no reduction, no atomics, no record.
#include "lsf_device.h"

using namespace lsf;

namespace {

typedef float vf4 __attribute__((ext_vector_type(4)));

template <int D>
__global__ __launch_bounds__(kBlock) void cumulative_warp_compose_kernel(const vf4* __restrict__ state,
                                                                         const vf4* __restrict__ psi_in,
                                                                         vf4* __restrict__ psi_out, Grid g, lsf_gate gate,
                                                                         const int* __restrict__ band_list,
                                                                         unsigned band_count) {
    // the gate of the iteration this launch follows: both read record i - 1 and take the same decision
    if (gate_closed(gate)) return;
    const vf4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for_each_listed_voxel(g, band_list, band_count, [&](int x, int y, int z) {
        const int i = vidx(g, x, y, z);
        const vf4 s = state[i];  // (live, u, v, w)
        // clamped before the integer conversion (axis_taps): a non-finite or huge update reads valid cells, as OOB taps
        const AxisTaps ax = axis_taps((float)x + s.y, g.nx, 0), ay = axis_taps((float)y + s.z, g.ny, 0);
        AxisTaps az = ax;
        if (D == 3) az = axis_taps((float)(z + g.z_global_offset) + s.w, g.nz, g.z_global_offset);
        auto tap = [&](int ox, int oy, int oz) {
            const long long idx = ((long long)(D == 3 ? (oz ? az.c1 : az.c0) : 0) * g.ny + (oy ? ay.c1 : ay.c0)) * g.nx +
                                  (ox ? ax.c1 : ax.c0);
            const bool valid = (ox ? ax.v1 : ax.v0) && (oy ? ay.v1 : ay.v0) && (D == 2 || (oz ? az.v1 : az.v0));
            const vf4 v = psi_in[idx];
            return valid ? v : zero;
        };
        vf4 c[2][2];  // [x offset][y offset] behind the z lerp
#pragma unroll
        for (int ox = 0; ox < 2; ++ox)
#pragma unroll
            for (int oy = 0; oy < 2; ++oy) {
                if (D == 3) {
                    const vf4 a = tap(ox, oy, 0), b = tap(ox, oy, 1);
                    c[ox][oy] = a * az.i + b * az.r;
                } else {
                    c[ox][oy] = tap(ox, oy, 0);
                }
            }
        const vf4 i0 = c[0][0] * ay.i + c[0][1] * ay.r;
        const vf4 i1 = c[1][0] * ay.i + c[1][1] * ay.r;
        const vf4 sampled = i0 * ax.i + i1 * ax.r;
        vf4 o;
        o.x = 0.0f;
        o.y = s.y + sampled.y;
        o.z = s.z + sampled.z;
        o.w = D == 3 ? s.w + sampled.w : 0.0f;
        psi_out[i] = o;  // what the next composition gathers from: still in L2 / MALL then
    });
}

}  // namespace

extern "C" int lsf_cumulative_warp_compose(const float* state, const float* psi_in, float* psi_out, const lsf_grid* grid,
                                           const lsf_gate* gate, const int32_t* band_list, int64_t band_count,
                                           void* stream) {
    // everything is checked before the launch, and every refusal is LSF_ERR_BAD_ARGUMENT (a grid check_grid turns down too)
    if (check_grid(grid)) return LSF_ERR_BAD_ARGUMENT;
    if (!state || !psi_in || !psi_out) return LSF_ERR_BAD_ARGUMENT;
    if ((uintptr_t)state % 16 || (uintptr_t)psi_in % 16 || (uintptr_t)psi_out % 16) return LSF_ERR_BAD_ARGUMENT;
    const size_t bytes = (size_t)grid->nz * grid->ny * grid->nx * 16;
    if (overlaps(psi_in, bytes, psi_out, bytes) || overlaps(state, bytes, psi_in, bytes) ||
        overlaps(state, bytes, psi_out, bytes))
        return LSF_ERR_BAD_ARGUMENT;
    // a list and its count go together: no list means the dense walk, which takes no count
    if (band_count < 0 || band_count > 0x7fffffffll || (band_list != nullptr) != (band_count > 0))
        return LSF_ERR_BAD_ARGUMENT;
    Grid g = make_grid(grid);
    Tiling t = make_tiling(g);
    if (t.total == 0) return 0;
    const unsigned blocks = band_list ? band_list_blocks((unsigned)band_count) : launch_blocks(t.total);
    const lsf_gate gt = gate_or_open(gate);
    if (grid->dims == 2)
        hipLaunchKernelGGL(cumulative_warp_compose_kernel<2>, dim3(blocks), dim3(kBlock), 0, as_stream(stream),
                           reinterpret_cast<const vf4*>(state), reinterpret_cast<const vf4*>(psi_in),
                           reinterpret_cast<vf4*>(psi_out), g, gt, band_list, (unsigned)band_count);
    else
        hipLaunchKernelGGL(cumulative_warp_compose_kernel<3>, dim3(blocks), dim3(kBlock), 0, as_stream(stream),
                           reinterpret_cast<const vf4*>(state), reinterpret_cast<const vf4*>(psi_in),
                           reinterpret_cast<vf4*>(psi_out), g, gt, band_list, (unsigned)band_count);
    return launch_status();
}
