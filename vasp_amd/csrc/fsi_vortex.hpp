// Q-criterion, enstrophy, helicity and kinetic energy of a recorded vector history on mesh cells, and their ordered weighted
// sums (fsi_vortex.hip): the launchers the C-ABI (fsi_band_cell_vortex and fsi_band_cell_vortex_current in fsi_sessions.hip)
// calls.  The lane state, the gather and the vertex gradients of k_cell_vortex and k_cell_vortex_current are those of
// fsi_cell.hpp, shared with the kernels of fsi_rate.hip.
//
// Compiler's resource report of k_cell_vortex for gfx950 (-Rpass-analysis=kernel-resource-usage): 256 VGPRs, 32 AGPRs, 46 SGPRs,
// no scratch, no LDS; one wave per SIMD - the thirty nodal values stay live to the end of a frame for the helicity and the
// kinetic energy, beside one vertex's gradient, the vertex sum and the twelve cell gradients.  Each vertex's gradient is
// consumed (Q, enstrophy and helicity sums) before the next vertex begins, so no more than one of the four is live.
// k_cell_wsum: 24 VGPRs, no AGPRs, 26 SGPRs, no scratch, 32 bytes of LDS; eight waves per SIMD.  k_cell_wsum_close: 38 VGPRs,
// 18 SGPRs, no scratch, no LDS.
// k_cell_vortex_current: 256 VGPRs, 80 AGPRs, 52 SGPRs, no scratch, no LDS; one wave per SIMD, as the two kernels it joins.  The
// seventy-two gradient entries of the field and the displacement and the field's thirty nodal values are live through the
// loop over the rule's fourteen points, 204 registers beside the lane's 44 and the eleven sums: what does not fit the 256
// VGPRs waits in AGPRs, which one wave per SIMD has free, and nothing goes to scratch.  The point loop is not unrolled - one
// point's temporaries are live at a time - and reads the rule and the basis values (kRule) through scalar loads.
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
// sums[f] = the ordered sum over the cells of weight[c] * value[f][c], f < nfield <= 64: per 256 cells a balanced tree over
// adjacent pairs inside each wave of 64, the four wave sums in wave order, then the workgroups' partials
// (partial[nfield][cell_wsum_blocks(n)]) in ascending order from +0.0.  Bit-equal to hi_pass.cell_wsum.
void launch_cell_wsum(hipStream_t st, int64_t n, int nfield, const double* weight, const double* value, double* partial, double* sums);
// launch_cell_vortex in the current configuration x = X + d(X): geo and geo_stride are the displacement's frames as x and
// frame_stride are the field's (launch_cell_rate_current).  out[12][n]: rows f < FSI_VORTEX_CURRENT_FIELDS the means over the
// frames of the means over the deformed cell r_0 .. r_4 and of the volume ratio Jbar; rows 6 + f the same means of the
// numerators n_0 .. n_4 (integrals per undeformed volume) and Jbar again, what launch_cell_wsum takes for the bulk sums.  The
// 14-point rule of degree 5 and the integrands: fsi_vortex.hip.  Bit-equal to hi_pass.cell_vortex_current.
void launch_cell_vortex_current(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                                const double* geo, int64_t geo_stride, int64_t count, double* out);

}  // namespace fsi
