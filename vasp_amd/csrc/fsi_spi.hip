// Spectral power index (SPI; Khan et al., J. Biomech. 2017) of a recorded history, on the device: per row the fraction of the
// non-mean spectral power that lies at or above a cut-off frequency.  The reference ships no tool for it (its spectrogram
// reader only prepares for one [REF src/vasp/postprocessing/postprocessing_h5py/spectrograms.py:203]).  The history is the
// band-pass session's (fsi_band.hip): x[frame][row], FP64, rows contiguous, here the session's selected raw frames.
//
// Only the kc lowest bins are transformed.  With Y[j] = w[j] (x[j] - mean), X_k = sum_j Y[j] exp(-2 pi i j k / n), by Parseval
//   AC  = n sum_j Y[j]^2 - |X_0|^2            all power but bin 0, two-sided
//   L   = 2 sum_{1 <= k < kc} |X_k|^2         the bins below the cut-off, both signs
//   SPI = (AC - L) / AC
//
//   k_spi_power : the geometry of k_spec_power (fsi_spec.hip) - a workgroup owns SPEC_ROWS rows, four waves of 16 bins each,
//                 SPEC_KC frames staged in LDS with Y formed while staging, Re = C Y and Im = S Y on v_mfma_f64_16x16x4_f64,
//                 D[bin = (lane >> 4) + 4 reg][row = lane & 15] - but the power is added per ROW over the bins: in a lane over
//                 the four registers of a tile, then over the four lane groups lane >> 4 (__shfl_xor 16, 32), kept per tile
//                 across the 64-bin passes, and at the end over the four waves through LDS in wave order.  Global bin 0 goes
//                 to a slot of its own.  The staging threads also add Y^2 of their row; the two threads of a row add in a
//                 fixed order.  Bins b >= nb carry zero table entries and add +0.0.  A row's values come from that row's
//                 column of Y alone: a NaN or an inf stays in its row.  The kernel runs one wave per SIMD, so nothing but
//                 its own instruction stream hides a load: the history, window and table entries of a chunk are loaded
//                 into registers while the chunk before is multiplied.
//   k_spi_close : one lane per node: AC, H = AC - L and the ratio per row, and the power-summed ratio per node of a vector.
//
// No atomics, contraction off: the same call gives the same bits.  The mean is k_spec_mean (launch_spec_mean, one segment).
#include "fsi_spi.hpp"
#include "fsi_spec.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int NT = SPEC_ROWS / 16;          // 16-row tiles per workgroup
constexpr int YLD = SPEC_ROWS + 16;         // LDS row stride [doubles], as k_spec_power: 288 dwords = 32 mod 64
constexpr int SJ = 256 / SPEC_ROWS;         // staging threads per row
static_assert(SPEC_BINS == 64 && SPEC_KC % 4 == 0 && SJ == 2 && SPEC_KC % SJ == 0, "k_spi_power: four waves x 16 bins, two staging threads per row");

__global__ __launch_bounds__(256) void k_spi_power(int64_t nrow, int64_t K, int64_t fstride, int64_t nb, int64_t bin0,
                                                   const double* __restrict__ x, const double* __restrict__ mean,
                                                   const double* __restrict__ w, const double* __restrict__ Ct,
                                                   const double* __restrict__ St, double* __restrict__ l2, double* __restrict__ x0,
                                                   double* __restrict__ q) {
  __shared__ double Ys[SPEC_KC][YLD];
  __shared__ double lows[4][SPEC_ROWS];     // the waves' sums over their low bins
  __shared__ double x0s[SPEC_ROWS];
  __shared__ double qs[SJ][SPEC_ROWS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * SPEC_ROWS;
  // staging: this thread forms the entries of row srow, frames sj, sj + SJ, ... of every chunk
  const int srow = t % SPEC_ROWS, sj = t / SPEC_ROWS;
  const bool rok = r0 + srow < nrow;
  const double mu = rok ? mean[r0 + srow] : 0.0;
  const bool first = bin0 == 0;
  double low[NT], dc[NT], qa = 0.0;
#pragma unroll
  for (int a = 0; a < NT; ++a) { low[a] = 0.0; dc[a] = 0.0; }
  for (int64_t b0 = 0; b0 < nb; b0 += SPEC_BINS) {
    v4d re[NT], im[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) { re[a] = v4d{0, 0, 0, 0}; im[a] = v4d{0, 0, 0, 0}; }
    const int64_t bcol = b0 + 16 * wave + lm;         // the bin this lane carries in the A fragment
    const bool bok = bcol < nb;
    const bool squares = first && b0 == 0;            // Y^2 is added in the first pass of the first slab
    // the history, window and table entries of a chunk are loaded into registers one chunk ahead, so that their latency
    // passes behind the products of the chunk before; every index is a constant after unrolling
    double xr[SPEC_KC / SJ], wr[SPEC_KC / SJ], cr[SPEC_KC / 4], sr[SPEC_KC / 4];
    auto fetch = [&](int64_t j0) {
#pragma unroll
      for (int i = 0; i < SPEC_KC / SJ; ++i) {
        const int64_t j = j0 + sj + SJ * i;
        const bool ok = rok && j < K;
        xr[i] = ok ? x[j * fstride + r0 + srow] : 0.0;
        wr[i] = (ok && w) ? w[j] : 1.0;
      }
#pragma unroll
      for (int kk = 0; kk < SPEC_KC / 4; ++kk) {
        const int64_t j = j0 + 4 * kk + lk;
        const bool ok = bok && j < K;
        cr[kk] = ok ? Ct[j * nb + bcol] : 0.0;
        sr[kk] = ok ? St[j * nb + bcol] : 0.0;
      }
    };
    fetch(0);
    for (int64_t j0 = 0; j0 < K; j0 += SPEC_KC) {
      __syncthreads();                                // the previous chunk has been read
#pragma unroll
      for (int i = 0; i < SPEC_KC / SJ; ++i) {
        const int jj = sj + SJ * i;
        const double y = (rok && j0 + jj < K) ? wr[i] * (xr[i] - mu) : 0.0;
        Ys[jj][srow] = y;
        if (squares) qa += y * y;
      }
      double c[SPEC_KC / 4], s[SPEC_KC / 4];
#pragma unroll
      for (int kk = 0; kk < SPEC_KC / 4; ++kk) { c[kk] = cr[kk]; s[kk] = sr[kk]; }
      if (j0 + SPEC_KC < K) fetch(j0 + SPEC_KC);
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < SPEC_KC / 4; ++kk) {
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const double y = Ys[4 * kk + lk][16 * a + lm];
          re[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(c[kk], y, re[a], 0, 0, 0);
          im[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(s[kk], y, im[a], 0, 0, 0);
        }
      }
    }
    // power of row 16 a + lm, added over the wave's 16 bins: the four registers, then the four lane groups
    const int64_t g0 = bin0 + b0 + 16 * wave + lk;   // the global bin of register 0
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      double p = 0.0, z = 0.0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const double pw = re[a][reg] * re[a][reg] + im[a][reg] * im[a][reg];
        if (reg == 0 && g0 == 0) z = pw;
        else p += pw;
      }
      p += __shfl_xor(p, 16);
      p += __shfl_xor(p, 32);
      z += __shfl_xor(z, 16);
      z += __shfl_xor(z, 32);
      low[a] += p;
      dc[a] += z;
    }
  }
  if (lk == 0) {
#pragma unroll
    for (int a = 0; a < NT; ++a) {
      lows[wave][16 * a + lm] = low[a];
      if (wave == 0) x0s[16 * a + lm] = dc[a];
    }
  }
  qs[sj][srow] = qa;
  __syncthreads();
  if (t < SPEC_ROWS && r0 + t < nrow) {
    const int64_t r = r0 + t;
    const double s = ((lows[0][t] + lows[1][t]) + lows[2][t]) + lows[3][t];
    if (first) {
      l2[r] = s;
      x0[r] = x0s[t];
      q[r] = qs[0][t] + qs[1][t];
    } else {
      l2[r] += s;
    }
  }
}

// H <= 0 ? 0 : H / AC: a row that is exactly constant (AC == 0) gives 0, a NaN fails the comparison and stays NaN
__device__ inline double spi_ratio(double H, double AC) { return H <= 0.0 ? 0.0 : H / AC; }

__global__ __launch_bounds__(256) void k_spi_close(int64_t nnode, int ncomp, double n, const double* __restrict__ l2,
                                                   const double* __restrict__ x0, const double* __restrict__ q,
                                                   double* __restrict__ rows, double* __restrict__ nodes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnode) return;
  double sH = 0.0, sAC = 0.0;
  for (int c = 0; c < ncomp; ++c) {
    const int64_t r = i * ncomp + c;
    const double AC = n * q[r] - x0[r], H = AC - 2.0 * l2[r];
    rows[r] = spi_ratio(H, AC);
    sH = c == 0 ? H : sH + H;
    sAC = c == 0 ? AC : sAC + AC;
  }
  nodes[i] = spi_ratio(sH, sAC);
}

}  // namespace

void launch_spi_power(hipStream_t st, int64_t nrow, int64_t K, int64_t stride, int64_t nb, int64_t bin0, const double* hist,
                      const double* mean, const double* w, const double* Ct, const double* St, double* l2, double* x0, double* q) {
  if (nrow > 0 && K > 0 && nb > 0)
    hipLaunchKernelGGL(k_spi_power, dim3((unsigned)spec_blocks(nrow)), dim3(256), 0, st, nrow, K, stride * nrow, nb, bin0, hist, mean, w,
                       Ct, St, l2, x0, q);
}

void launch_spi_close(hipStream_t st, int64_t nnode, int ncomp, int64_t n, const double* l2, const double* x0, const double* q,
                      double* rows, double* nodes) {
  if (nnode > 0)
    hipLaunchKernelGGL(k_spi_close, dim3((unsigned)((nnode + 255) / 256)), dim3(256), 0, st, nnode, ncomp, (double)n, l2, x0, q, rows, nodes);
}

}  // namespace fsi
