// Band-pass filtered fields and windowed RMS amplitudes of a run, on the device (the h5py post-processing).
//
// Replaces the per-node Python loops of vasp-create-hi-pass-viz
// [REF src/vasp/postprocessing/postprocessing_h5py/create_hi_pass_viz.py:190-215,218-230,370-403;
//  spectrograms.py:502-555 (butter_bandpass_filter -> scipy.signal.filtfilt); postprocessing_h5py_common.py:685-731
//  (calculate_windowed_rms)] on a history that is recorded while the run steps: hist[frame][row], FP64, a row being one
// (node, component) of the Visualization writer's node list.  Frame-major, so that with one lane per row every time step
// of every wavefront is one contiguous 512-byte access.
//
//   k_band_sample    : hist[frame][row] = U[idx0[row]] (or the mean of two entries: the pressure of an edge node of the
//                      save_deg 2 output).  One contiguous write, no atomics.
//   k_band_filter    : scipy.signal.filtfilt(b, a, x) per row, operation by operation: the odd extension by padlen samples
//                      at both ends (2 x[0] - x[padlen - j], 2 x[n-1] - x[n-2-k]) formed on the fly, lfilter's transposed
//                      direct form II
//                          y      = z[0] + b[0] x
//                          z[k]   = z[k+1] + x b[k+1] - y a[k+1]          (evaluated left to right)
//                          z[m-1] = x b[m] - y a[m]
//                      started from zi * ext[0] forward (into work) and from zi * y[-1] backward (in place).  The state is
//                      ten doubles in registers.  The filter is ill-conditioned (order 10, lower edge at 1 / 400 of the sampling
//                      rate: an ulp in the input moves the output by 1e-5 of the filtered signal), so a reformulated recurrence
//                      would give other numbers than the tool this replaces: floating-point contraction is off in this file,
//                      and FP64 multiply / add / subtract are correctly rounded, which reproduces the host bit for bit.
//                      Loads run UNR frames ahead of the recurrence: the dependency chain is y -> z[0] -> y (three FP64
//                      operations per sample), not the memory system.  Its input is a view of the history: frames first,
//                      first + stride, ... (the launcher offsets the pointer, xs is the distance of two selected frames).
//   k_band_filter_next: the same filtfilt of the filtered series itself, y <- filtfilt(b, a, y), inside work: stage k of a
//                      multiband cascade (create_hi_pass_viz.py:191-198).  The forward pass overwrites its input as it goes:
//                      the head of the extension reads ahead of the write position, the body reads the element it is about
//                      to overwrite, and only the tail extension needs inputs that are gone - the last padlen + 1 samples,
//                      kept per lane in LDS (34 x 64 doubles, 17 KiB; indexed by a loop counter, which registers cannot be).
//   k_band_trace     : the rows of a few listed nodes over all selected frames, raw or filtered, with their magnitude
//                      (create_point_trace, postprocessing_h5py_common.py:470-483): out[point][frame][1 + ncomp].
//   k_band_rms       : flat-window RMS sqrt(convolve(y^2, ones(w) / w, "valid")), frame by frame: the sum of squares of a
//                      window is advanced from the previous window's (+ newest^2 - oldest^2) and recomputed exactly every
//                      BAND_RMS_REFRESH windows, so that rounding cannot accumulate; clamped at zero before the square root
//                      - an amplitude is never NaN.
//   k_band_magnitude : |amplitude| over the three components per node (numpy.linalg.norm's order), k_band_argmax_* its
//                      maximum and the first node that has it (create_hi_pass_viz.py:341,381,390).
//   k_band_select    : exact order statistics of a frame at up to SEL_MAX_RANKS ranks (the neighbours of the table's
//                      percentiles, create_hi_pass_viz.py:377-390): a most-significant-digit radix select on the
//                      order-preserving 64-bit image of the FP64 bits, one workgroup per frame, eight passes of one byte.
//                      Ranks whose images still share their leading bytes share one LDS histogram of 256 integer counts; a
//                      pass adds every element whose leading bytes are a rank's to that histogram (integer LDS atomics: the
//                      counts, and so the result, do not depend on the order the lanes arrive in), then one lane per rank
//                      walks its histogram to the byte its rank falls in.  Magnitudes of one frame share their leading
//                      bytes, so a lane sums a run of equal slots in a register and adds once per run, not once per element.
#include "fsi_band.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

constexpr int UNR = 8;          // frames of loads in flight per lane
constexpr int NZ = BAND_MAX_TAPS - 1;

__device__ __forceinline__ double band_step(const BandCoef& c, double (&z)[NZ], double x) {
  const double y = z[0] + c.b[0] * x;
#pragma unroll
  for (int k = 0; k < NZ - 1; ++k) z[k] = (z[k + 1] + x * c.b[k + 1]) - y * c.a[k + 1];
  z[NZ - 1] = x * c.b[NZ] - y * c.a[NZ];
  return y;
}

// the second half of filtfilt: the forward result w[0 .. L) filtered from its last sample to its first, in place
__device__ __forceinline__ void band_backward(const BandCoef& c, double (&z)[NZ], double* w, int64_t nrow, int64_t L) {
  {
    const double yl = w[(L - 1) * nrow];
#pragma unroll
    for (int k = 0; k < NZ; ++k) z[k] = c.zi[k] * yl;
  }
  for (int64_t j0 = L - 1; j0 >= 0; j0 -= UNR) {
    double v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) v[u] = j0 - u >= 0 ? w[(j0 - u) * nrow] : 0.0;
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (j0 - u >= 0) w[(j0 - u) * nrow] = band_step(c, z, v[u]);
  }
}

__global__ __launch_bounds__(256) void k_band_sample(int64_t nrow, const double* __restrict__ U, const int32_t* __restrict__ idx0,
                                                     const int32_t* __restrict__ idx1, double* __restrict__ dst) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrow) return;
  const int32_t j = idx1[r];
  const double a = U[idx0[r]];
  dst[r] = j < 0 ? a : 0.5 * (a + U[j]);
}

__global__ __launch_bounds__(64) void k_band_filter(int64_t nrow, int64_t n, int p, BandCoef c, const double* __restrict__ hist,
                                                    int64_t xs, double* __restrict__ work) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= nrow) return;
  const int64_t L = n + 2 * (int64_t)p;
  const double* x = hist + r;
  double* w = work + r;
  const double x0 = x[0], xl = x[(n - 1) * xs];
  double z[NZ];
  {
    const double e0 = 2.0 * x0 - x[(int64_t)p * xs];
#pragma unroll
    for (int k = 0; k < NZ; ++k) z[k] = c.zi[k] * e0;
  }
  for (int64_t j0 = 0; j0 < L; j0 += UNR) {          // forward over the extended series
    double v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t j = j0 + u;                      // uniform over the wavefront
      if (j < p) v[u] = 2.0 * x0 - x[(p - j) * xs];
      else if (j < p + n) v[u] = x[(j - p) * xs];
      else if (j < L) v[u] = 2.0 * xl - x[(n - 2 - (j - p - n)) * xs];
      else v[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (j0 + u < L) w[(j0 + u) * nrow] = band_step(c, z, v[u]);
  }
  band_backward(c, z, w, nrow, L);
}

// The series is x[i] = w[(q + i) nrow], i < n, left by a stage of padlen q >= p; the result takes w[0 .. n + 2 p), the series at
// w[p ..].  One pointer: input and output alias.  A batch's loads are all issued before its stores, and every load of a batch
// is at or ahead of the batch's first store (head: q + p - j > j for j < p <= q; body: q + j - p >= j), so no load sees a
// value of this stage.
__global__ __launch_bounds__(64) void k_band_filter_next(int64_t nrow, int64_t n, int q, int p, BandCoef c, double* work) {
  __shared__ double tail[BAND_MAX_PADLEN + 1][64];   // tail[k][lane] = x[n - 1 - p + k], k <= p: a lane reads its own column only
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= nrow) return;
  const int lane = threadIdx.x;
  const int64_t L = n + 2 * (int64_t)p;
  double* w = work + r;
  const double* x = w + (int64_t)q * nrow;
  const double x0 = x[0], xl = x[(n - 1) * nrow];
  for (int k = 0; k <= p; ++k) tail[k][lane] = x[(n - 1 - p + k) * nrow];      // n > p: the index is >= 0
  double z[NZ];
  {
    const double e0 = 2.0 * x0 - x[(int64_t)p * nrow];
#pragma unroll
    for (int k = 0; k < NZ; ++k) z[k] = c.zi[k] * e0;
  }
  for (int64_t j0 = 0; j0 < L; j0 += UNR) {          // forward over the extended series, over its own input
    double v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t j = j0 + u;                      // uniform over the wavefront
      if (j < p) v[u] = 2.0 * x0 - x[(p - j) * nrow];
      else if (j < p + n) v[u] = x[(j - p) * nrow];
      else if (j < L) v[u] = 2.0 * xl - tail[p - 1 - (j - p - n)][lane];       // x[n - 2 - (j - p - n)]
      else v[u] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (j0 + u < L) w[(j0 + u) * nrow] = band_step(c, z, v[u]);
  }
  band_backward(c, z, w, nrow, L);
}

__global__ __launch_bounds__(256) void k_band_trace(int64_t total, int64_t nframes, int ncomp, const int32_t* __restrict__ points,
                                                    const double* __restrict__ src, int64_t xs, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (point, frame)
  if (i >= total) return;
  const double* x = src + (i % nframes) * xs + (int64_t)ncomp * points[i / nframes];
  double* o = out + i * (1 + ncomp);
  if (ncomp == 3) {
    const double a = x[0], b = x[1], c = x[2];
    o[0] = sqrt((a * a + b * b) + c * c);
    o[1] = a; o[2] = b; o[3] = c;
  } else {
    o[0] = x[0];
    o[1] = x[0];
  }
}

__global__ __launch_bounds__(256) void k_band_rms(int64_t nrow, const double* __restrict__ y, int64_t start, int window, int recompute,
                                                  double* __restrict__ acc, double* __restrict__ amp) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrow) return;
  double s;
  if (recompute) {
    s = 0.0;
    for (int64_t j = start; j < start + window; ++j) {
      const double v = y[j * nrow + r];
      s += v * v;
    }
  } else {
    const double v1 = y[(start + window - 1) * nrow + r], v0 = y[(start - 1) * nrow + r];
    s = (acc[r] + v1 * v1) - v0 * v0;
  }
  acc[r] = s;
  amp[r] = sqrt(fmax(s, 0.0) / (double)window);      // fmax(NaN, 0) = 0
}

__global__ __launch_bounds__(256) void k_band_magnitude(int64_t nnode, int ncomp, const double* __restrict__ amp,
                                                        double* __restrict__ mag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnode) return;
  if (ncomp == 3) {
    const double a = amp[3 * i], b = amp[3 * i + 1], c = amp[3 * i + 2];
    mag[i] = sqrt((a * a + b * b) + c * c);
  } else {
    mag[i] = amp[i];
  }
}

// numpy.argmax: the first index of the largest value
__device__ __forceinline__ void take_max(double& bv, int64_t& bi, double v, int64_t i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__device__ __forceinline__ void block_argmax(double& bv, int64_t& bi) {
  __shared__ double sv[256];
  __shared__ int64_t si[256];
  const int t = threadIdx.x;
  sv[t] = bv;
  si[t] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) take_max(sv[t], si[t], sv[t + s], si[t + s]);
    __syncthreads();
  }
  bv = sv[0];
  bi = si[0];
}

__global__ __launch_bounds__(256) void k_band_argmax_part(int64_t n, const double* __restrict__ mag, double* __restrict__ pv,
                                                          int64_t* __restrict__ pi) {
  double bv = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) take_max(bv, bi, mag[i], i);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) { pv[1 + blockIdx.x] = bv; pi[1 + blockIdx.x] = bi; }
}

__global__ __launch_bounds__(256) void k_band_argmax_final(int nparts, double* __restrict__ pv, int64_t* __restrict__ pi) {
  double bv = -INFINITY;
  int64_t bi = INT64_MAX;
  for (int k = threadIdx.x; k < nparts; k += 256) take_max(bv, bi, pv[1 + k], pi[1 + k]);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) { pv[0] = bv; pi[0] = bi == INT64_MAX ? 0 : bi; }
}

// The image orders as the values do: sign bit flipped for v >= +0, every bit for v < 0 (-0 lies below +0); a NaN of either
// sign takes the largest image, behind +inf, where numpy.sort puts it.
__device__ __forceinline__ uint64_t sel_image(double v) {
  if (v != v) return ~0ull;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double sel_value(uint64_t k) {
  if (k == ~0ull) return __longlong_as_double(0x7FF8000000000000ll);
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

// x[frame][.] at distance xs; ranks[nr] ascending and distinct, 0 <= rank < n; out[frame][nr], nans[frame]
__global__ __launch_bounds__(256) void k_band_select(int64_t n, int64_t xs, const double* __restrict__ x, int nr,
                                                     const int64_t* __restrict__ ranks, double* __restrict__ out,
                                                     int64_t* __restrict__ nans) {
  __shared__ uint32_t hist[BAND_SEL_MAX_RANKS][256];     // one per group of ranks with the same leading bytes
  __shared__ uint64_t prefix[BAND_SEL_MAX_RANKS];        // per rank: the leading bytes found so far
  __shared__ uint64_t below[BAND_SEL_MAX_RANKS];         // per rank: its rank among the elements that have those bytes
  __shared__ uint64_t gprefix[BAND_SEL_MAX_RANKS];       // per group
  __shared__ int group_of[BAND_SEL_MAX_RANKS];
  __shared__ int ngroups;
  __shared__ uint32_t nan_count;
  const int t = threadIdx.x;
  const double* f = x + (int64_t)blockIdx.x * xs;
  if (t < nr) { prefix[t] = 0; below[t] = (uint64_t)ranks[t]; }
  if (t == 0) nan_count = 0;
  __syncthreads();
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (t == 0) {
      int g = 0;
      for (int r = 0; r < nr; ++r) {
        if (r == 0 || prefix[r] != prefix[r - 1]) gprefix[g++] = prefix[r];
        group_of[r] = g - 1;
      }
      ngroups = g;
    }
    __syncthreads();
    const int ng = ngroups;
    for (int k = t; k < ng * 256; k += 256) (&hist[0][0])[k] = 0;
    __syncthreads();
    int slot = -1;                  // a run of elements for one slot of the histograms: summed here, added once
    uint32_t run = 0, my_nans = 0;
    for (int64_t i = t; i < n; i += 256) {
      const double v = f[i];
      const uint64_t key = sel_image(v);
      if (pass == 0 && v != v) ++my_nans;
      int g = 0;
      if (pass > 0) {
        const uint64_t lead = key >> (shift + 8);
        for (g = 0; g < ng; ++g)
          if (gprefix[g] == lead) break;
        if (g == ng) continue;      // no rank lies among the elements with these leading bytes
      }
      const int s = g * 256 + (int)((key >> shift) & 255);
      if (s != slot) {
        if (run) atomicAdd(&(&hist[0][0])[slot], run);
        slot = s;
        run = 0;
      }
      ++run;
    }
    if (run) atomicAdd(&(&hist[0][0])[slot], run);
    if (pass == 0 && my_nans) atomicAdd(&nan_count, my_nans);
    __syncthreads();
    if (t < nr) {
      const uint32_t* h = hist[group_of[t]];
      uint64_t k = below[t], c = 0;
      int d = 0;
      for (; d < 255; ++d) {        // the byte d with c(d) <= k < c(d) + h[d]; every element is counted, so one exists
        if (k < c + h[d]) break;
        c += h[d];
      }
      prefix[t] = (prefix[t] << 8) | (uint64_t)d;
      below[t] = k - c;
    }
    __syncthreads();
  }
  if (t < nr) out[(int64_t)blockIdx.x * nr + t] = sel_value(prefix[t]);
  if (t == 0) nans[blockIdx.x] = (int64_t)nan_count;
}

}  // namespace

void launch_band_sample(hipStream_t st, int64_t nrow, const double* U, const int32_t* idx0, const int32_t* idx1, double* dst) {
  if (nrow > 0) hipLaunchKernelGGL(k_band_sample, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, nrow, U, idx0, idx1, dst);
}

void launch_band_filter(hipStream_t st, int64_t nrow, int64_t nframes, int padlen, const BandCoef& c, const double* hist,
                        int64_t stride, double* work) {
  if (nrow > 0)
    hipLaunchKernelGGL(k_band_filter, dim3((unsigned)((nrow + 63) / 64)), dim3(64), 0, st, nrow, nframes, padlen, c, hist, stride * nrow, work);
}

void launch_band_filter_next(hipStream_t st, int64_t nrow, int64_t nframes, int padlen_prev, int padlen, const BandCoef& c, double* work) {
  if (nrow > 0)
    hipLaunchKernelGGL(k_band_filter_next, dim3((unsigned)((nrow + 63) / 64)), dim3(64), 0, st, nrow, nframes, padlen_prev, padlen, c, work);
}

void launch_band_trace(hipStream_t st, int64_t nrow, int ncomp, int64_t npoints, const int32_t* points, int64_t nframes,
                       const double* src, int64_t stride, double* out) {
  const int64_t total = npoints * nframes;
  if (total > 0)
    hipLaunchKernelGGL(k_band_trace, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, nframes, ncomp, points, src, stride * nrow, out);
}

void launch_band_rms(hipStream_t st, int64_t nrow, const double* y, int64_t start, int window, bool recompute, double* acc,
                     double* amp) {
  if (nrow > 0)
    hipLaunchKernelGGL(k_band_rms, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, nrow, y, start, window, recompute ? 1 : 0, acc, amp);
}

void launch_band_magnitude(hipStream_t st, int64_t nnode, int ncomp, const double* amp, double* mag) {
  if (nnode > 0) hipLaunchKernelGGL(k_band_magnitude, dim3((unsigned)((nnode + 255) / 256)), dim3(256), 0, st, nnode, ncomp, amp, mag);
}

void launch_band_argmax(hipStream_t st, int64_t n, const double* mag, double* part_val, int64_t* part_idx) {
  if (n <= 0) return;
  const int nb = (int)((n + 255) / 256 < BAND_ARGMAX_BLOCKS ? (n + 255) / 256 : BAND_ARGMAX_BLOCKS);
  hipLaunchKernelGGL(k_band_argmax_part, dim3(nb), dim3(256), 0, st, n, mag, part_val, part_idx);
  hipLaunchKernelGGL(k_band_argmax_final, dim3(1), dim3(256), 0, st, nb, part_val, part_idx);
}

void launch_band_select(hipStream_t st, int64_t n, int64_t nframes, int64_t stride, const double* x, int nranks, const int64_t* ranks,
                        double* out, int64_t* nans) {
  if (n > 0 && nframes > 0 && nranks > 0)
    hipLaunchKernelGGL(k_band_select, dim3((unsigned)nframes), dim3(256), 0, st, n, stride, x, nranks, ranks, out, nans);
}

}  // namespace fsi
