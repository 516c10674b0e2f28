// Average spectrograms and power spectra of a recorded history (fsi_spec.hip): tile sizes and the launchers the C-ABI
// (fsi_spec_* in fsi_sessions.hip) calls.  The history is the band-pass session's: src[frame][row], FP64, rows contiguous.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

constexpr int SPEC_ROWS = 128;     // rows (columns of Y) a workgroup owns: eight 16-wide tiles of v_mfma_f64_16x16x4_f64
constexpr int SPEC_BINS = 64;      // frequency bins per workgroup pass: four waves x one 16-bin tile
constexpr int SPEC_KC = 16;        // frames staged in LDS per step
constexpr int64_t SPEC_MAX_NFFT = 1ll << 26;      // transform lengths the host makes cos / sin tables for (1 GiB of angles)

// tmp[c * n + i] (three sampled components, component-major) -> dst[i] = sqrt((x^2 + y^2) + z^2)
void launch_spec_magnitude(hipStream_t st, int64_t n, const double* tmp, double* dst);
// mean[seg][row] = (x[seg * step][row] + ... + x[seg * step + K - 1][row]) / K, summed in frame order; with stride > 1 the
// K frames of a segment are x[seg * step + j * stride], j < K
void launch_spec_mean(hipStream_t st, int64_t nrow, int64_t K, int64_t step, int64_t nseg, const double* x, double* mean,
                      int64_t stride = 1);
// part[seg][block][b] = sum over the rows of block `block` (SPEC_ROWS rows each, in a fixed order) of
//   factor(b) * scale * ((C Y)^2 + (S Y)^2)[b][row],  Y[j][row] = w[j] * (x[seg * step + j][row] - mean[seg][row]),
// for the nb bins of a slab.  Ct / St: [K][nb], the slab's cos / sin columns, frame-major.  factor(b) = 1 for global bin
// bin0 + b == 0 and for bin0 + b == last_single (the Nyquist bin of an even nfft, -1 if none), 2 otherwise.
void launch_spec_power(hipStream_t st, int64_t nrow, int64_t K, int64_t step, int64_t nseg, int64_t nb, int64_t bin0,
                       int64_t last_single, double scale, const double* x, const double* mean, const double* w,
                       const double* Ct, const double* St, double* part);
// out[(bin0 + b) * nseg + seg] = (part[seg][0][b] + part[seg][1][b] + ...) / nrow, the blocks added in index order
void launch_spec_reduce(hipStream_t st, int64_t nrow, int64_t nseg, int64_t nb, int64_t bin0, const double* part, double* out);
// The same additions for a session that holds rows first_row .. first_row + nrow - 1 of a longer list (first_row a multiple of
// SPEC_ROWS): s = first_row > 0 ? carry[(bin0 + b) * nseg + seg] : +0.0, s += part[seg][0][b], part[seg][1][b], ...;
// carry[...] = s, or s / total_rows where total_rows > 0 (the last strip).  No atomics: one thread per (bin, segment).
void launch_spec_reduce_sum(hipStream_t st, int64_t nrow, int64_t nseg, int64_t nb, int64_t bin0, int64_t first_row, int64_t total_rows,
                            const double* part, double* carry);

inline int64_t spec_blocks(int64_t nrow) { return (nrow + SPEC_ROWS - 1) / SPEC_ROWS; }

}  // namespace fsi
