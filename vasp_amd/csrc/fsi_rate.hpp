// Cell means of the strain rate of a recorded vector history (fsi_rate.hip): the launchers the C-ABI (fsi_band_cells,
// fsi_band_cell_rate in fsi_sessions.hip) calls.
//
// Compiler's resource report of k_cell_rate for gfx950 (-Rpass-analysis=kernel-resource-usage): 180 VGPRs, no AGPRs, 22 SGPRs,
// no scratch, no LDS; two waves per SIMD.  (With the frame loop's invariants - the 78 products of the gradient values with the
// basis coefficients of the restated expression - kept in registers it took 256 VGPRs and 68 AGPRs, one wave per SIMD; see the
// comment in cell_rate_of and DESIGN.md section 8.)
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

}  // namespace fsi
