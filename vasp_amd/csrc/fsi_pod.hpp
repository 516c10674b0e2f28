// Snapshot proper orthogonal decomposition of a recorded history (fsi_pod.hip): the launchers the C-ABI (fsi_band_pod_gram,
// fsi_band_pod_modes, fsi_band_pod_fetch in fsi_sessions.hip) calls.  The history is the band-pass session's: frames of nrow
// doubles, rows contiguous, `fstride` doubles from one taken frame to the next - the selected raw frames through the
// selection's stride, or the filtered series behind its guard frames.  The mean is k_spec_mean (launch_spec_mean, one segment).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fsi {

constexpr int POD_FB = 64;            // frames of a frame block: four waves x one 16-frame strip of v_mfma_f64_16x16x4_f64
constexpr int POD_CHUNK = 128;        // rows staged in LDS per step
constexpr int POD_SLAB = 6144;        // rows of a slab: 48 chunks, a multiple of 3 - the summation order depends on (rows, frames) alone
constexpr int POD_MAX_MODES = 64;     // modes of one k_pod_modes launch: four waves x one 16-mode tile
constexpr int64_t POD_MAX_FRAMES = 16384;      // 256 frame blocks, 32 896 block pairs: the second grid dimension
static_assert(POD_SLAB % 3 == 0 && POD_SLAB % POD_CHUNK == 0, "a slab is whole chunks and whole nodes of a vector");

inline int64_t pod_frame_blocks(int64_t n) { return (n + POD_FB - 1) / POD_FB; }
inline int64_t pod_pairs(int64_t n) { const int64_t b = pod_frame_blocks(n); return b * (b + 1) / 2; }      // block pairs bi <= bj
inline int64_t pod_slabs(int64_t nrow) { return (nrow + POD_SLAB - 1) / POD_SLAB; }
// doubles of the partial tiles part[slab][pair][POD_FB][POD_FB]
inline size_t pod_part_count(int64_t nrow, int64_t n) { return (size_t)pod_slabs(nrow) * (size_t)pod_pairs(n) * POD_FB * POD_FB; }

// With y_j[row] = x[j * fstride + row] - mean[row], j < n, and a_j[row] = w[row] * y_j[row] (w null: a_j = y_j, no product):
//   part[slab][pair (bi, bj)][i][j] = sum over the slab's rows, ascending, of a_(64 bi + i)[row] * y_(64 bj + j)[row]
// with frames >= n counted as +0.0.  Plain stores: every slot is written.
void launch_pod_gram(hipStream_t st, int64_t nrow, int64_t n, int64_t fstride, const double* x, const double* mean, const double* w,
                     double* part);
// G[i][j] = G[j][i] = ((+0.0 + part[0][..]) + part[1][..]) + ... over the slabs in ascending order, for i <= j < n: G[n][n]
void launch_pod_gram_close(hipStream_t st, int64_t nrow, int64_t n, const double* part, double* G);
// modes[m][row] = sum_j T[j * nmodes + m] * y_j[row], m < nmodes <= POD_MAX_MODES, j < n in ascending groups of four
void launch_pod_modes(hipStream_t st, int64_t nrow, int64_t n, int64_t fstride, int64_t nmodes, const double* x, const double* mean,
                      const double* T, double* modes);

}  // namespace fsi
