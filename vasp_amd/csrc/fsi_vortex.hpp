// Q-criterion, enstrophy, helicity and kinetic energy of a recorded vector history on mesh cells, and their ordered weighted
// sums (fsi_vortex.hip): the launchers the C-ABI (fsi_band_cell_vortex in fsi_sessions.hip) calls.  The lane state, the gather
// and the vertex gradient of k_cell_vortex are those of fsi_cell.hpp, shared with the kernels of fsi_rate.hip.
//
// Compiler's resource report of k_cell_vortex for gfx950 (-Rpass-analysis=kernel-resource-usage): 256 VGPRs, 32 AGPRs, 46 SGPRs,
// no scratch, no LDS; one wave per SIMD - the thirty nodal values stay live to the end of a frame for the helicity and the
// kinetic energy, beside one vertex's gradient, the vertex sum and the twelve cell gradients.  Each vertex's gradient is
// consumed (Q, enstrophy and helicity sums) before the next vertex begins, so no more than one of the four is live.
// k_cell_wsum: 24 VGPRs, no AGPRs, 20 SGPRs, no scratch, 32 bytes of LDS; eight waves per SIMD.  k_cell_wsum_close: 38 VGPRs,
// 18 SGPRs, no scratch, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vaspfsi.h"

namespace fsi {

// out[f][c], f < FSI_VORTEX_FIELDS, = (((+0.0 + r_0) + r_1) + ...) / count with r_k field f of frame k of the P2 field w whose
// node a of cell c is the triple x[k * frame_stride + 3 * conn[c][a] ..]; conn[n][10] and gl[n][4][3] as launch_cell_rate takes
// them.  Every field is an exact cell mean (the fields and their order: fsi_vortex.hip).  Bit-equal to hi_pass.cell_vortex.
void launch_cell_vortex(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                        int64_t count, double* out);
// the workgroups of launch_cell_wsum: 256 consecutive cells each
inline int64_t cell_wsum_blocks(int64_t n) { return (n + 255) / 256; }
// sums[f] = the ordered sum over the cells of weight[c] * value[f][c], f < FSI_VORTEX_FIELDS: per 256 cells a balanced tree over
// adjacent pairs inside each wave of 64, the four wave sums in wave order, then the workgroups' partials
// (partial[FSI_VORTEX_FIELDS][cell_wsum_blocks(n)]) in ascending order from +0.0.  Bit-equal to hi_pass.cell_wsum.
void launch_cell_wsum(hipStream_t st, int64_t n, const double* weight, const double* value, double* partial, double* sums);

}  // namespace fsi
