// Cell means of the strain rate of a recorded vector history (fsi_rate.hip): the launchers the C-ABI (fsi_band_cells,
// fsi_band_cell_rate, fsi_band_cell_rate_current in fsi_sessions.hip) calls.
//
// The lane state, the gather and the vertex gradient are those of fsi_cell.hpp, shared with k_cell_vortex (fsi_vortex.hip).
//
// Compiler's resource report of k_cell_rate for gfx950 (-Rpass-analysis=kernel-resource-usage): 180 VGPRs, no AGPRs, 20 SGPRs,
// no scratch, no LDS; two waves per SIMD.  (With the frame loop's invariants - the 78 products of the gradient values with the
// basis coefficients of vertex_gradient_of - kept in registers it took 256 VGPRs and 68 AGPRs, one wave per SIMD; see the
// comment at fence_cell_gradients (fsi_cell.hpp) and DESIGN.md section 8.)
//
// The same report of k_cell_rate_current: 256 VGPRs, 22 AGPRs, 28 SGPRs, no scratch, no LDS; one wave per SIMD.  The vertex
// gradients are formed one vertex after the other (vertex_gradients_of makes each vertex's nine values opaque before the next
// begins, fence_vertex_gradient): left to the scheduler, the 36 x 22 independent products are formed ahead of their sums and
// the kernel takes all 512 registers and 332 bytes of scratch per lane.  Asking for two waves per SIMD costs 92 bytes of
// scratch, so it is one wave.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

// gl[c][4][3]: the physical gradients of the four barycentric coordinates of cell cells[c], from geom[C][10] (the undeformed
// geometry, rows of Jinv): gl[1 .. 3] = rows 0 .. 2, gl[0] = -((row 0 + row 1) + row 2), as wss_dg1_cell forms them
void launch_cell_gradients(hipStream_t st, int64_t n, const double* geom, const int32_t* cells, double* gl);
// out[c] = (((+0.0 + r_0) + r_1) + ...) / count with r_k the exact cell mean of 2 S:S, S = sym(grad w), of the P2 field w whose
// node a of cell c is the triple x[k * frame_stride + 3 * conn[c][a] ..]: conn[n][10] indices of nodes within a frame, local
// order (vertices, then the edges {2,3},{1,3},{1,2},{0,3},{0,2},{0,1}); gl[n][4][3] of launch_cell_gradients
void launch_cell_rate(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                      int64_t count, double* out);
// launch_cell_rate in the current configuration x = X + d(X): frame k of the field is x[k * frame_stride ..], that of the
// displacement geo[k * geo_stride ..], both on the nodes of conn.  Per frame r = (sum_q J_q e_q) / (sum_q J_q) over the four
// points of the degree-2 interior rule, e_q = 2 S_q:S_q with S_q = sym(G_q adj(F_q) / J_q), F_q = I + D_q, J_q = det F_q.
// rate[c]: the ordered mean of r as launch_cell_rate forms it; volume_ratio[c]: the same of 0.25 sum_q J_q; min_jacobian[c]:
// the smallest J_q met, from +inf, a NaN never taken.  Bit-equal to hi_pass.cell_rate_current.
void launch_cell_rate_current(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                              const double* geo, int64_t geo_stride, int64_t count, double* rate, double* volume_ratio,
                              double* min_jacobian);

}  // namespace fsi
