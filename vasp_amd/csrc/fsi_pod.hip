// Snapshot proper orthogonal decomposition (POD) of a recorded history, on the device: the Gram matrix of the mean-free frames
// in a weighted inner product, and the modes from a table the host forms of the Gram matrix's eigenvectors.  The reference
// ships no tool for it.  The history is the band-pass session's (fsi_band.hip): x[frame][row], FP64, rows contiguous - the
// selected raw frames through the selection's stride, or the series that stands.
//
// With m the ordered mean of a row over the n frames, y_j = x_j - m and a_j = w y_j (w the weight of the row's node; none: a_j
// is y_j itself):   G[i][j] = sum_r a_i[r] y_j[r],   Phi_m[r] = sum_j T[j][m] y_j[r].
//
//   k_pod_gram       : every matrix kernel here keeps rows independent and reduces over frames; this one reduces over the rows.
//                      The rows are cut into slabs of POD_SLAB, the frames into blocks of POD_FB = 64; a workgroup owns one slab
//                      and one pair of frame blocks bi <= bj and walks the slab in ascending chunks of POD_CHUNK rows.  The two
//                      blocks of a chunk are staged in LDS frame by frame - loads coalesced along the rows - with the mean taken
//                      off and the weight put on the i side only while staging; frames >= n and rows past the slab are +0.0.  A
//                      diagonal pair loads its block once.  On v_mfma_f64_16x16x4_f64 the k index is four consecutive rows:
//                      A[m = frame i = lane & 15][k = row = lane >> 4], B[k = row = lane >> 4][n = frame j = lane & 15],
//                      D[i = (lane >> 4) + 4 reg][j = lane & 15].  A wave keeps its 16-frame strip of the i block against the four
//                      16-frame tiles of the j block in registers for the whole slab; the next chunk is loaded into registers
//                      while the current one multiplies, as in k_spi_power.  The slab's tile goes to part[slab][pair] by plain
//                      stores.  The summation order is a function of (rows, frames) alone.
//   k_pod_gram_close : one lane per (i, j), i <= j: the slabs' partials added in ascending order from +0.0, stored to G[i][j] and
//                      G[j][i] - G is symmetric bit for bit.
//   k_pod_modes      : the geometry of k_spi_power - 128 rows a workgroup, four waves of 16 modes, 16 frames staged in LDS with y
//                      formed while staging - with the host's table T in the place of the cosine table and the raw product
//                      stored, modes[m][row].  Modes >= nmodes carry zero table entries and are not stored.
//
// No atomics, contraction off: the same call gives the same bits.  The mean is k_spec_mean (launch_spec_mean, one segment).
#include "fsi_pod.hpp"
#include "fsi_spec.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

// LDS row stride of a staged frame [doubles].  A fragment read takes, per 32-lane half, 16 frames (lane & 15) x 2 consecutive
// rows (lane >> 4): with a stride of 2 mod 32 doubles - 4 mod 64 dwords - frame f starts at bank 4 f, so the 32 lanes of a
// half cover the 64 banks once, as k_spi_power's YLD does for its 16 rows x 2 frames with 32 mod 64 dwords.  The staging
// writes run along a frame: consecutive doubles.
constexpr int POD_LD = POD_CHUNK + 2;
constexpr int GJ = 256 / POD_CHUNK;           // staging threads per row
constexpr int GL = POD_FB / GJ;               // frames of a block a staging thread carries
static_assert(POD_FB == 64 && POD_CHUNK % 4 == 0 && GJ == 2 && POD_LD % 32 == 2, "k_pod_gram: four waves x 16 frames, two staging threads per row");

__global__ __launch_bounds__(256) void k_pod_gram(int64_t nrow, int64_t n, int64_t fstride, int nfb, const double* __restrict__ x,
                                                  const double* __restrict__ mean, const double* __restrict__ w,
                                                  double* __restrict__ part) {
  __shared__ double As[POD_FB][POD_LD];       // a_i of the i block's frames
  __shared__ double Bs[POD_FB][POD_LD];       // y_j of the j block's frames
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lk = lane >> 4;
  int bi = 0, bj = (int)blockIdx.y;           // pair index -> (bi, bj), bi <= bj, row by row of the upper triangle
  while (bj >= nfb - bi) { bj -= nfb - bi; ++bi; }
  bj += bi;
  const bool diag = bi == bj;
  const int64_t r_begin = (int64_t)blockIdx.x * POD_SLAB, r_end = r_begin + POD_SLAB < nrow ? r_begin + POD_SLAB : nrow;
  // staging: this thread forms the entries of row srow, frames sj, sj + GJ, ... of both blocks of every chunk
  const int srow = t % POD_CHUNK, sj = t / POD_CHUNK;
  const int64_t fi0 = (int64_t)POD_FB * bi + sj, fj0 = (int64_t)POD_FB * bj + sj;
  v4d acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) acc[a] = v4d{0, 0, 0, 0};
  // the history, mean and weight of a chunk are loaded into registers one chunk ahead; every index is a constant after unrolling
  double xi[GL], xj[GL], mu = 0.0, wt = 1.0;
  auto fetch = [&](int64_t r0) {
    const int64_t r = r0 + srow;
    const bool rok = r < r_end;
    mu = rok ? mean[r] : 0.0;
    wt = (rok && w) ? w[r] : 1.0;
#pragma unroll
    for (int i = 0; i < GL; ++i) {
      const int64_t f = fi0 + GJ * i;
      xi[i] = (rok && f < n) ? x[f * fstride + r] : 0.0;
    }
    if (!diag) {
#pragma unroll
      for (int i = 0; i < GL; ++i) {
        const int64_t f = fj0 + GJ * i;
        xj[i] = (rok && f < n) ? x[f * fstride + r] : 0.0;
      }
    }
  };
  fetch(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += POD_CHUNK) {
    __syncthreads();                                // the previous chunk has been read
    const bool rok = r0 + srow < r_end;
#pragma unroll
    for (int i = 0; i < GL; ++i) {
      const int jj = sj + GJ * i;
      const bool oki = rok && fi0 + GJ * i < n;
      const double yi = oki ? xi[i] - mu : 0.0;
      As[jj][srow] = (oki && w) ? wt * yi : yi;
      if (diag) Bs[jj][srow] = yi;
      else Bs[jj][srow] = (rok && fj0 + GJ * i < n) ? xj[i] - mu : 0.0;
    }
    if (r0 + POD_CHUNK < r_end) fetch(r0 + POD_CHUNK);
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < POD_CHUNK / 4; ++kk) {
      const double a = As[16 * wave + lm][4 * kk + lk];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[16 * tt + lm][4 * kk + lk], acc[tt], 0, 0, 0);
    }
  }
  double* out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (POD_FB * POD_FB);
#pragma unroll
  for (int tt = 0; tt < 4; ++tt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(16 * wave + lk + 4 * reg) * POD_FB + 16 * tt + lm] = acc[tt][reg];
}

__global__ __launch_bounds__(256) void k_pod_gram_close(int64_t n, int64_t nfb, int64_t nslab, const double* __restrict__ part,
                                                        double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * n) return;
  const int64_t i = e / n, j = e % n;
  if (i > j) return;
  const int64_t bi = i / POD_FB, bj = j / POD_FB, npairs = nfb * (nfb + 1) / 2;
  const int64_t pair = bi * nfb - bi * (bi - 1) / 2 + (bj - bi);
  const double* p = part + (size_t)pair * (POD_FB * POD_FB) + (i % POD_FB) * POD_FB + j % POD_FB;
  double s = 0.0;
  for (int64_t slab = 0; slab < nslab; ++slab) s += p[(size_t)slab * (size_t)npairs * (POD_FB * POD_FB)];
  G[i * n + j] = s;
  G[j * n + i] = s;
}

constexpr int NT = SPEC_ROWS / 16;          // 16-row tiles per workgroup
constexpr int YLD = SPEC_ROWS + 16;         // LDS row stride [doubles], as k_spi_power: 288 dwords = 32 mod 64
constexpr int SJ = 256 / SPEC_ROWS;         // staging threads per row
static_assert(POD_MAX_MODES == 64 && SPEC_KC % 4 == 0 && SJ == 2 && SPEC_KC % SJ == 0, "k_pod_modes: four waves x 16 modes, two staging threads per row");

__global__ __launch_bounds__(256) void k_pod_modes(int64_t nrow, int64_t K, int64_t fstride, int64_t nmodes, const double* __restrict__ x,
                                                   const double* __restrict__ mean, const double* __restrict__ T,
                                                   double* __restrict__ modes) {
  __shared__ double Ys[SPEC_KC][YLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lm = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * SPEC_ROWS;
  // staging: this thread forms the entries of row srow, frames sj, sj + SJ, ... of every chunk
  const int srow = t % SPEC_ROWS, sj = t / SPEC_ROWS;
  const bool rok = r0 + srow < nrow;
  const double mu = rok ? mean[r0 + srow] : 0.0;
  const int64_t mcol = 16 * wave + lm;        // the mode this lane carries in the A fragment
  const bool mok = mcol < nmodes;
  v4d phi[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a) phi[a] = v4d{0, 0, 0, 0};
  // the history and table entries of a chunk are loaded into registers one chunk ahead, as in k_spi_power
  double xr[SPEC_KC / SJ], tr[SPEC_KC / 4];
  auto fetch = [&](int64_t j0) {
#pragma unroll
    for (int i = 0; i < SPEC_KC / SJ; ++i) {
      const int64_t j = j0 + sj + SJ * i;
      xr[i] = (rok && j < K) ? x[j * fstride + r0 + srow] : 0.0;
    }
#pragma unroll
    for (int kk = 0; kk < SPEC_KC / 4; ++kk) {
      const int64_t j = j0 + 4 * kk + lk;
      tr[kk] = (mok && j < K) ? T[j * nmodes + mcol] : 0.0;
    }
  };
  fetch(0);
  for (int64_t j0 = 0; j0 < K; j0 += SPEC_KC) {
    __syncthreads();                                // the previous chunk has been read
#pragma unroll
    for (int i = 0; i < SPEC_KC / SJ; ++i) {
      const int jj = sj + SJ * i;
      Ys[jj][srow] = (rok && j0 + jj < K) ? xr[i] - mu : 0.0;
    }
    double c[SPEC_KC / 4];
#pragma unroll
    for (int kk = 0; kk < SPEC_KC / 4; ++kk) c[kk] = tr[kk];
    if (j0 + SPEC_KC < K) fetch(j0 + SPEC_KC);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SPEC_KC / 4; ++kk) {
#pragma unroll
      for (int a = 0; a < NT; ++a) phi[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(c[kk], Ys[4 * kk + lk][16 * a + lm], phi[a], 0, 0, 0);
    }
  }
  // D[mode = (lane >> 4) + 4 reg][row = lane & 15] of tile a
#pragma unroll
  for (int a = 0; a < NT; ++a) {
    const int64_t r = r0 + 16 * a + lm;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t m = 16 * wave + lk + 4 * reg;
      if (m < nmodes && r < nrow) modes[m * nrow + r] = phi[a][reg];
    }
  }
}

}  // namespace

void launch_pod_gram(hipStream_t st, int64_t nrow, int64_t n, int64_t fstride, const double* x, const double* mean, const double* w,
                     double* part) {
  if (nrow > 0 && n > 0)
    hipLaunchKernelGGL(k_pod_gram, dim3((unsigned)pod_slabs(nrow), (unsigned)pod_pairs(n)), dim3(256), 0, st, nrow, n, fstride,
                       (int)pod_frame_blocks(n), x, mean, w, part);
}

void launch_pod_gram_close(hipStream_t st, int64_t nrow, int64_t n, const double* part, double* G) {
  if (nrow > 0 && n > 0)
    hipLaunchKernelGGL(k_pod_gram_close, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, n, pod_frame_blocks(n), pod_slabs(nrow), part, G);
}

void launch_pod_modes(hipStream_t st, int64_t nrow, int64_t n, int64_t fstride, int64_t nmodes, const double* x, const double* mean,
                      const double* T, double* modes) {
  if (nrow > 0 && n > 0 && nmodes > 0)
    hipLaunchKernelGGL(k_pod_modes, dim3((unsigned)spec_blocks(nrow)), dim3(256), 0, st, nrow, n, fstride, nmodes, x, mean, T, modes);
}

}  // namespace fsi
