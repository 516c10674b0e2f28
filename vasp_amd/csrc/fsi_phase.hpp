// Phase-averaged (Reynolds) decomposition of a recorded history and the energy of its fluctuation (fsi_phase.hip): the
// launchers the C-ABI (fsi_band_phase, fsi_band_phase_fetch in fsi_sessions.hip) calls.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

constexpr int PHASE_REG_CYCLES = 8;                    // up to this many cycles a lane keeps its values in registers

// x[k][row] = hist[k * stride][row], k < cycles * period (the launcher is handed the first selected frame):
//   mean[j][row]              = (((+0.0 + x[j]) + x[period + j]) + ...) / cycles,  j < period
//   fluct[c * period + j][row] = x[c * period + j][row] - mean[j][row]
// hist is read once for cycles <= PHASE_REG_CYCLES and twice above; 16-byte accesses where nrow is even.
void launch_phase_decompose(hipStream_t st, int64_t nrow, int64_t period, int64_t cycles, const double* hist, int64_t stride,
                            double* mean, double* fluct);
// the energy e = 0.5 * ((fx fx + fy fy) + fz fz) per node (ncomp 3) or 0.5 * (f f) (ncomp 1) of fluctuation frames
// f[t * step][.], t < terms, a frame being [nnode][ncomp]: out[node] = e of the one frame (mean false, terms 1) or
// (((+0.0 + e[0]) + e[1]) + ...) / terms
void launch_phase_energy(hipStream_t st, int64_t nnode, int ncomp, const double* f, int64_t step, int64_t terms, bool mean, double* out);

}  // namespace fsi
