// Strain rate of a recorded velocity (or displacement) history on mesh cells, on the device: what the flow and simulation
// metrics of a run are formed from - viscous and turbulent dissipation, Kolmogorov scales, l+ and t+ (vasp_amd/flow_metrics.py).
//
// Replaces nothing in the reference; VaMPy computes these metrics for a rigid-wall run, here they are formed on the history a
// band-pass session holds (hist[frame][row], a node's three components contiguous).
//
//   k_cell_gl   : the gradients of a listed cell's barycentric coordinates from the context's undeformed geometry, once per
//                 cell list.
//   k_cell_rate : one lane per listed cell.  The lane keeps the cell's ten node indices and its twelve gradient values in
//                 registers and walks `count` frames of one series.  Per frame it gathers the ten nodes' triples (240 B), forms
//                 G_t = grad w at the four vertices t - the gradient of a P2 field is linear on the cell, so they determine it;
//                 the expression is that of wss_dg1_cell (fsi_wss.hpp), restated -, S_t = 0.5 (G_t + G_t^T) and
//                 r = 0.1 * (sum_t S_t:S_t + (sum_t S_t):(sum_t S_t)), the exact cell mean of 2 S:S, since the integral of
//                 L_a L_b over the cell is |K| (1 + delta_ab) / 20.  out = (((+0.0 + r_0) + r_1) + ...) / count: the sum in frame
//                 order, a true division; one frame gives its own bits.  NaN and inf propagate, nothing is clamped.
//
// No LDS, no atomics, FP64 vector loads and stores.  Floating-point contraction is off, as in fsi_band.hip and fsi_phase.hip:
// the NumPy twin (hi_pass.cell_rate) rounds every product and every sum, and the device equals it bit for bit.
#include "fsi_rate.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

__global__ __launch_bounds__(256) void k_cell_gl(int64_t n, const double* __restrict__ geom, const int32_t* __restrict__ cells,
                                                 double* __restrict__ gl) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double* Jg = geom + (int64_t)cells[c] * 10;
  double* g = gl + c * 12;
  for (int j = 0; j < 3; ++j) {
    g[3 + j] = Jg[j]; g[6 + j] = Jg[3 + j]; g[9 + j] = Jg[6 + j];
    g[j] = -((Jg[j] + Jg[3 + j]) + Jg[6 + j]);
  }
}

// the cell mean of 2 sym(grad w):sym(grad w): w[a][i] component i of local node a, gl[a][j] the gradient of barycentric
// coordinate a.  Every operation in the order of hi_pass.cell_rate.
__device__ __forceinline__ double cell_rate_of(const double (&w)[10][3], double (&gl)[4][3]) {
  const int E[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
  double q = 0.0, T[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[i][j] = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    // The products of the gradient values with the basis coefficients below do not depend on the frame: left alone, the
    // compiler forms all 78 of them once and keeps them in registers across the frame loop (256 VGPRs + 68 AGPRs, one wave per
    // SIMD).  Making gl opaque here has them formed again per vertex and frame - a quarter more multiplications, the same bits -
    // and leaves room for two waves per SIMD, which the gather needs to hide its latency.
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(gl[a][j]));
    double G[3][3];                                   // grad w at vertex t
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) s = s + w[a][i] * ((a == t ? 3.0 : -1.0) * gl[a][j]);
#pragma unroll
        for (int e = 0; e < 6; ++e) {
          const int p = E[e][0], r = E[e][1];
          s = s + (w[4 + e][i] * 4.0) * ((p == t ? 1.0 : 0.0) * gl[r][j] + (r == t ? 1.0 : 0.0) * gl[p][j]);
        }
        G[i][j] = s;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double S = 0.5 * (G[i][j] + G[j][i]);
        q = q + S * S;
        T[i][j] = T[i][j] + S;
      }
  }
  double p = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) p = p + T[i][j] * T[i][j];
  return 0.1 * (q + p);
}

__global__ __launch_bounds__(256) void k_cell_rate(int64_t n, const int32_t* __restrict__ conn, const double* __restrict__ gl_all,
                                                   const double* __restrict__ x, int64_t frame_stride, int64_t count,
                                                   double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  int64_t row[10];
#pragma unroll
  for (int a = 0; a < 10; ++a) row[a] = 3 * (int64_t)conn[c * 10 + a];
  double gl[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 3; ++j) gl[a][j] = gl_all[c * 12 + a * 3 + j];
  double s = 0.0;
  for (int64_t k = 0; k < count; ++k) {
    const double* f = x + k * frame_stride;
    double w[10][3];
#pragma unroll
    for (int a = 0; a < 10; ++a)
#pragma unroll
      for (int i = 0; i < 3; ++i) w[a][i] = f[row[a] + i];
    s = s + cell_rate_of(w, gl);
  }
  out[c] = s / (double)count;
}

}  // namespace

void launch_cell_gradients(hipStream_t st, int64_t n, const double* geom, const int32_t* cells, double* gl) {
  if (n > 0) hipLaunchKernelGGL(k_cell_gl, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, geom, cells, gl);
}

void launch_cell_rate(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                      int64_t count, double* out) {
  if (n > 0 && count > 0)
    hipLaunchKernelGGL(k_cell_rate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, conn, gl, x, frame_stride, count, out);
}

}  // namespace fsi
