// Average spectrograms and power spectra of a run, on the device (the h5py post-processing).
//
// Replaces the per-row Python loops of vasp-create-spectrograms-chromagrams and vasp-create-spectrum
// [REF src/vasp/postprocessing/postprocessing_h5py/spectrograms.py:397-421 (get_psd -> scipy.signal.periodogram),
//  :424-473 (get_spectrogram -> scipy.signal.spectrogram), :558-583 (filter_time_data)] on a history that is recorded while
// the run steps, in the band-pass session's layout (fsi_band.hip): x[frame][row], FP64, rows contiguous.  Recording and
// filtering ARE that file's launch_band_sample / launch_band_filter.  What is here is the short-time transform and the
// average over the rows:
//
//   k_spec_magnitude : the |.| of a sampled vector, taken at sample time (component "mag").
//   k_spec_mean      : the mean of every (segment, row) over its K frames, added in frame order: scipy's
//                      detrend="constant", the default of spectrogram and periodogram alike.  The frames of a segment may
//                      lie `stride` recorded frames apart (the selected view of a band-pass session, fsi_spi.hip).
//   k_spec_power     : for one segment and SPEC_ROWS rows, Re = C Y and Im = S Y on v_mfma_f64_16x16x4_f64, with
//                      Y[j][row] = w[j] (x[j][row] - mean[row]) formed while the tile is staged in LDS - the window and the
//                      detrend are never folded into the table: a folded table would move the cancellation of a 1e4 Pa mean
//                      into the dot product.  C / S[k][j] = cos / sin(2 pi (j k mod nfft) / nfft) come from the host in
//                      FP64, stored frame-major ([j][k]) so that the A fragment of a wave is four 128-byte runs, like its B
//                      fragment.  Only the K frames of a segment are multiplied: zero-padding to nfft > K costs nothing.
//                      Operand layout: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15],
//                      D[row = (lane >> 4) + 4 reg][col = lane & 15] (tools/mfma_layout_check.hip).  A wave owns 16 bins x
//                      SPEC_ROWS rows: 8 + 8 accumulator tiles.  The power (Re^2 + Im^2) scale of a row is added over the
//                      wave's rows in a fixed order (tile by tile in a lane, then a four-step butterfly over the 16 lanes of
//                      a bin) and written as the workgroup's partial sum - one slot per (segment, row block, bin).
//   k_spec_reduce    : adds the row blocks' partial sums in index order and divides by the number of rows; its carried
//                      variant starts from the sum of the row blocks before the session's first row and hands the sum on
//                      (fsi_spec_spectrogram_sum / fsi_spec_periodogram_sum: a history in strips of rows).
//
// No floating-point atomics anywhere: the same call gives the same bits.  A periodogram is one segment of all n frames
// with nfft = n; the C-ABI hands the tables over in slabs of bins (nb, bin0) so that a long run's table never has to fit.
#include "fsi_spec.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int NT = SPEC_ROWS / 16;          // 16-row tiles per workgroup
constexpr int YLD = SPEC_ROWS + 16;         // LDS row stride [doubles]: 288 dwords = 32 mod 64, so the two frames a 32-lane
                                            // half of a ds_read_b64 touches lie on disjoint banks
static_assert(SPEC_BINS == 64 && SPEC_KC % 4 == 0 && 256 % SPEC_ROWS == 0, "k_spec_power: four waves x 16 bins, 256 threads");

__global__ __launch_bounds__(256) void k_spec_magnitude(int64_t n, const double* __restrict__ tmp, double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = tmp[i], b = tmp[n + i], c = tmp[2 * n + i];
  dst[i] = sqrt((a * a + b * b) + c * c);
}

__global__ __launch_bounds__(256) void k_spec_mean(int64_t nrow, int64_t K, int64_t step, int64_t pitch, const double* __restrict__ x,
                                                   double* __restrict__ mean) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  if (r >= nrow) return;
  const double* xs = x + seg * step * nrow + r;
  double s = 0.0;
  for (int64_t j = 0; j < K; ++j) s += xs[j * pitch];
  mean[seg * nrow + r] = s / (double)K;
}

__global__ __launch_bounds__(256) void k_spec_power(int64_t nrow, int64_t K, int64_t step, int64_t nb, int64_t bin0,
                                                    int64_t last_single, double scale, const double* __restrict__ x,
                                                    const double* __restrict__ mean, const double* __restrict__ w,
                                                    const double* __restrict__ Ct, const double* __restrict__ St,
                                                    double* __restrict__ part) {
  __shared__ double Ys[SPEC_KC][YLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lk = lane >> 4;
  const int64_t blk = blockIdx.x, seg = blockIdx.y, nblk = gridDim.x, r0 = blk * SPEC_ROWS;
  const double* xs = x + seg * step * nrow;
  // staging: this thread forms the entries of row srow, frames sj, sj + SJ, ... of every chunk
  constexpr int SJ = 256 / SPEC_ROWS;
  const int srow = t % SPEC_ROWS, sj = t / SPEC_ROWS;
  const bool rok = r0 + srow < nrow;
  const double mu = rok ? mean[seg * nrow + r0 + srow] : 0.0;
  for (int64_t b0 = 0; b0 < nb; b0 += SPEC_BINS) {
    v4d re[NT], im[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) { re[a] = v4d{0, 0, 0, 0}; im[a] = v4d{0, 0, 0, 0}; }
    const int64_t bcol = b0 + 16 * wave + lm;         // the bin this lane carries in the A fragment
    const bool bok = bcol < nb;
    for (int64_t j0 = 0; j0 < K; j0 += SPEC_KC) {
      __syncthreads();                                // the previous chunk has been read
#pragma unroll
      for (int i = 0; i < SPEC_KC / SJ; ++i) {
        const int jj = sj + SJ * i;
        const int64_t j = j0 + jj;
        Ys[jj][srow] = (rok && j < K) ? w[j] * (xs[j * nrow + r0 + srow] - mu) : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < SPEC_KC / 4; ++kk) {
        const int64_t j = j0 + 4 * kk + lk;
        const bool ok = bok && j < K;
        const double c = ok ? Ct[j * nb + bcol] : 0.0, s = ok ? St[j * nb + bcol] : 0.0;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const double y = Ys[4 * kk + lk][16 * a + lm];
          re[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(c, y, re[a], 0, 0, 0);
          im[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(s, y, im[a], 0, 0, 0);
        }
      }
    }
    // power of the wave's 16 bins, added over the workgroup's rows: tile by tile, then over the 16 lanes of a bin
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      double p = 0.0;
#pragma unroll
      for (int a = 0; a < NT; ++a) p += (re[a][reg] * re[a][reg] + im[a][reg] * im[a][reg]) * scale;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off, 16);
      const int64_t b = b0 + 16 * wave + lk + 4 * reg;
      if (lm == 0 && b < nb) {
        const int64_t g = bin0 + b;
        part[(seg * nblk + blk) * nb + b] = (g == 0 || g == last_single) ? p : 2.0 * p;
      }
    }
  }
}

// CARRY = false: out = the mean over the nrow rows of this session.  CARRY = true (a session that holds rows first_row ... of
// total_rows, fsi_spec_*_sum): the sum starts from what out holds of the row blocks before first_row - from +0.0 with
// first_row == 0, as above -, goes on over this session's blocks and is written back; told the total (total_rows > 0, the
// last strip) the mean over that many rows is written over it.  One body: the additions are those of one call on all rows.
template <bool CARRY>
__global__ __launch_bounds__(256) void k_spec_reduce(int64_t nrow, int64_t nblk, int64_t nseg, int64_t nb, int64_t bin0, int64_t first_row,
                                                     int64_t total_rows, const double* __restrict__ part, double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  if (b >= nb) return;
  const int64_t o = (bin0 + b) * nseg + seg;
  double s = 0.0;
  if (CARRY && first_row > 0) s = out[o];
  for (int64_t k = 0; k < nblk; ++k) s += part[(seg * nblk + k) * nb + b];
  if (CARRY) {
    out[o] = s;
    if (total_rows > 0) out[o] = s / (double)total_rows;
  } else {
    out[o] = s / (double)nrow;
  }
}

}  // namespace

void launch_spec_magnitude(hipStream_t st, int64_t n, const double* tmp, double* dst) {
  if (n > 0) hipLaunchKernelGGL(k_spec_magnitude, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, tmp, dst);
}

void launch_spec_mean(hipStream_t st, int64_t nrow, int64_t K, int64_t step, int64_t nseg, const double* x, double* mean, int64_t stride) {
  if (nrow > 0 && nseg > 0)
    hipLaunchKernelGGL(k_spec_mean, dim3((unsigned)((nrow + 255) / 256), (unsigned)nseg), dim3(256), 0, st, nrow, K, step, stride * nrow, x, mean);
}

void launch_spec_power(hipStream_t st, int64_t nrow, int64_t K, int64_t step, int64_t nseg, int64_t nb, int64_t bin0,
                       int64_t last_single, double scale, const double* x, const double* mean, const double* w,
                       const double* Ct, const double* St, double* part) {
  if (nrow > 0 && nseg > 0 && nb > 0)
    hipLaunchKernelGGL(k_spec_power, dim3((unsigned)spec_blocks(nrow), (unsigned)nseg), dim3(256), 0, st, nrow, K, step, nb, bin0,
                       last_single, scale, x, mean, w, Ct, St, part);
}

void launch_spec_reduce(hipStream_t st, int64_t nrow, int64_t nseg, int64_t nb, int64_t bin0, const double* part, double* out) {
  if (nrow > 0 && nseg > 0 && nb > 0)
    hipLaunchKernelGGL(k_spec_reduce<false>, dim3((unsigned)((nb + 255) / 256), (unsigned)nseg), dim3(256), 0, st, nrow, spec_blocks(nrow),
                       nseg, nb, bin0, (int64_t)0, (int64_t)0, part, out);
}

void launch_spec_reduce_sum(hipStream_t st, int64_t nrow, int64_t nseg, int64_t nb, int64_t bin0, int64_t first_row, int64_t total_rows,
                            const double* part, double* carry) {
  if (nrow > 0 && nseg > 0 && nb > 0)
    hipLaunchKernelGGL(k_spec_reduce<true>, dim3((unsigned)((nb + 255) / 256), (unsigned)nseg), dim3(256), 0, st, nrow, spec_blocks(nrow),
                       nseg, nb, bin0, first_row, total_rows, part, carry);
}

}  // namespace fsi
