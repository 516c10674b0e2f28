// Phase-averaged (Reynolds) decomposition of a run's recorded history and the turbulent kinetic energy of its fluctuation,
// on the device, for every written node.
//
// Replaces compute_tke and compute_average_over_cycles of vasp-log-plotter [REF src/vasp/postprocessing/log_plotter.py:
// 902-925,928-989], which the reference can apply only to the few probe points a problem file prints into its log.  The
// input is the view of a band-pass session's history hist[frame][row] that fsi_band_select holds: n = C * P frames, C
// cycles of P frames each.
//
//   k_phase_decompose : mean[j][row] = (((+0.0 + x[j]) + x[P + j]) + ...) / C and fluct[c P + j][row] = x[c P + j][row] -
//                       mean[j][row]: the reference's sum over the cycles in cycle order, its true division and its
//                       subtraction.  Pure streaming: rows are contiguous within a frame, one lane owns one row (two where
//                       the row count is even: 16-byte accesses; with an odd count every second frame starts 8 bytes off a
//                       16-byte boundary) at one phase j.  Up to PHASE_REG_CYCLES cycles a lane keeps its C values in
//                       registers, so hist is read once: n rows 8 bytes in, (n + P) rows 8 bytes out.  Above, it reads them
//                       a second time for the subtraction.
//   k_phase_energy    : e = 0.5 * ((fx fx + fy fy) + fz fz) per node of one fluctuation frame, or the sum of e over frames
//                       t * step, t < terms, in order from +0.0, divided by terms: the mean over the cycles at one phase
//                       (step = P frames) and the mean over all frames (step = one frame).  Formed when fetched: no
//                       n x nodes array of energies exists.
//
// Floating-point contraction is off, as in fsi_band.hip: a fused x * x + y * y rounds once where the reference rounds twice.
#include "fsi_phase.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ double vsub(double a, double b) { return a - b; }
__device__ __forceinline__ double vdiv(double a, double d) { return a / d; }
__device__ __forceinline__ double vzero(const double*) { return 0.0; }
__device__ __forceinline__ double2 vadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 vsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 vdiv(double2 a, double d) { return make_double2(a.x / d, a.y / d); }
__device__ __forceinline__ double2 vzero(const double2*) { return make_double2(0.0, 0.0); }

// units: lanes per frame (rows, or pairs of rows); xs, fs: the distance of two selected frames in hist and of two frames in
// mean / fluct, in elements of V.  REG: the cycles' values stay in registers, needs C <= REG; 0: they are read twice.
template <int REG, class V>
__global__ __launch_bounds__(256) void k_phase_decompose(int64_t units, int64_t P, int64_t C, const V* __restrict__ hist, int64_t xs,
                                                         int64_t fs, V* __restrict__ mean, V* __restrict__ fluct) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // (phase, unit)
  if (i >= P * units) return;
  const int64_t j = i / units, r = i - j * units;
  const V* x = hist + j * xs + r;
  V* f = fluct + j * fs + r;
  const int64_t xc = P * xs, fc = P * fs;                                // one cycle on
  const double count = (double)C;
  V s = vzero(x);
  if constexpr (REG > 0) {
    V v[REG];
#pragma unroll
    for (int c = 0; c < REG; ++c)
      if (c < C) v[c] = x[c * xc];
#pragma unroll
    for (int c = 0; c < REG; ++c)
      if (c < C) s = vadd(s, v[c]);
    const V m = vdiv(s, count);
    mean[j * fs + r] = m;
#pragma unroll
    for (int c = 0; c < REG; ++c)
      if (c < C) f[c * fc] = vsub(v[c], m);
  } else {
    for (int64_t c = 0; c < C; ++c) s = vadd(s, x[c * xc]);
    const V m = vdiv(s, count);
    mean[j * fs + r] = m;
    for (int64_t c = 0; c < C; ++c) f[c * fc] = vsub(x[c * xc], m);
  }
}

__global__ __launch_bounds__(256) void k_phase_energy(int64_t nnode, int ncomp, const double* __restrict__ f, int64_t step, int64_t terms,
                                                      int mean, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnode) return;
  const double* p = f + (int64_t)ncomp * i;
  double s = 0.0, e = 0.0;
  for (int64_t t = 0; t < terms; ++t) {
    if (ncomp == 3) {
      const double a = p[t * step], b = p[t * step + 1], c = p[t * step + 2];
      e = 0.5 * ((a * a + b * b) + c * c);
    } else {
      const double a = p[t * step];
      e = 0.5 * (a * a);
    }
    s = s + e;
  }
  out[i] = mean ? s / (double)terms : e;
}

template <class V>
void decompose(hipStream_t st, int64_t units, int64_t P, int64_t C, const V* hist, int64_t xs, V* mean, V* fluct) {
  const dim3 grid((unsigned)((P * units + 255) / 256)), block(256);
  if (C <= PHASE_REG_CYCLES) hipLaunchKernelGGL((k_phase_decompose<PHASE_REG_CYCLES, V>), grid, block, 0, st, units, P, C, hist, xs, units, mean, fluct);
  else hipLaunchKernelGGL((k_phase_decompose<0, V>), grid, block, 0, st, units, P, C, hist, xs, units, mean, fluct);
}

}  // namespace

void launch_phase_decompose(hipStream_t st, int64_t nrow, int64_t period, int64_t cycles, const double* hist, int64_t stride,
                            double* mean, double* fluct) {
  if (nrow <= 0 || period <= 0 || cycles <= 0) return;
  if (nrow % 2 == 0)          // every frame of hist, mean and fluct starts on a 16-byte boundary
    decompose(st, nrow / 2, period, cycles, reinterpret_cast<const double2*>(hist), stride * (nrow / 2), reinterpret_cast<double2*>(mean),
              reinterpret_cast<double2*>(fluct));
  else
    decompose(st, nrow, period, cycles, hist, stride * nrow, mean, fluct);
}

void launch_phase_energy(hipStream_t st, int64_t nnode, int ncomp, const double* f, int64_t step, int64_t terms, bool mean, double* out) {
  if (nnode > 0 && terms > 0)
    hipLaunchKernelGGL(k_phase_energy, dim3((unsigned)((nnode + 255) / 256)), dim3(256), 0, st, nnode, ncomp, f, step, terms, mean ? 1 : 0, out);
}

}  // namespace fsi
