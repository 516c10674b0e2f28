// Spectral power index of a recorded history, per row and per node (fsi_spi.hip): the launchers the C-ABI (fsi_band_spi,
// fsi_band_spi_fetch in fsi_sessions.hip) calls.  Tile sizes and the mean are those of fsi_spec.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

// x[j][row] = hist[j * stride][row], j < K (the launcher is handed the first selected frame; a frame has nrow rows):
//   Y[j][row] = w[j] * (x[j][row] - mean[row])      (w null: the boxcar, Y = x - mean)
// and, for the nb bins of a slab whose cos / sin columns are Ct / St [K][nb], frame-major, global bin g = bin0 + b:
//   l2[row] (+)= sum over the slab's bins g >= 1 of (C Y)^2 + (S Y)^2    (= with bin0 == 0, += with bin0 > 0)
//   x0[row]  = (C Y)^2 + (S Y)^2 of bin g == 0                            (bin0 == 0 only)
//   q[row]   = sum_j Y[j][row]^2                                          (bin0 == 0 only)
// Every sum in a fixed order; a row's three values depend on that row alone.
void launch_spi_power(hipStream_t st, int64_t nrow, int64_t K, int64_t stride, int64_t nb, int64_t bin0, const double* hist,
                      const double* mean, const double* w, const double* Ct, const double* St, double* l2, double* x0, double* q);
// Per row: AC = n q - x0, H = AC - 2 l2, rows[row] = H <= 0 ? 0 : H / AC (a NaN stays one).  Per node, ncomp 3:
// nodes[node] = sH <= 0 ? 0 : sH / sAC with sH = (H_0 + H_1) + H_2 and sAC likewise; ncomp 1: the row's value.
void launch_spi_close(hipStream_t st, int64_t nnode, int ncomp, int64_t n, const double* l2, const double* x0, const double* q,
                      double* rows, double* nodes);

}  // namespace fsi
