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
//                 the lane state, the gather and the expression are those of fsi_cell.hpp -, S_t = 0.5 (G_t + G_t^T) and
//                 r = 0.1 * (sum_t S_t:S_t + (sum_t S_t):(sum_t S_t)), the exact cell mean of 2 S:S, since the integral of
//                 L_a L_b over the cell is |K| (1 + delta_ab) / 20.  out = (((+0.0 + r_0) + r_1) + ...) / count: the sum in frame
//                 order, a true division; one frame gives its own bits.  NaN and inf propagate, nothing is clamped.
//
//   k_cell_rate_current : the same in the current configuration x = X + d(X) of an ALE run: one lane per listed cell walks
//                 `count` frames of a field w and of the displacement d together (480 B gathered per cell and frame).  With
//                 G_t and D_t the vertex gradients of w and d in the undeformed geometry, at the four points of the degree-2
//                 interior rule - weight a = 0.5854101966249685 on vertex q, b = 0.1381966011250105 on the other three, so
//                 G_q = b (sum_t G_t) + (a - b) G_q, exact for a gradient that is linear on the cell -: F_q = I + D_q,
//                 J_q = det F_q, L_q = G_q adj(F_q) / J_q, S_q = 0.5 (L_q + L_q^T), e_q = 2 S_q:S_q, and the frame's value
//                 r = (sum_q J_q e_q) / (sum_q J_q), the mean over the deformed cell (with d = 0 the rule is exact and r is the
//                 r of k_cell_rate to rounding).  Three results per cell: rate, the mean of r over the frames as k_cell_rate
//                 forms it; volume_ratio, the same ordered mean of 0.25 sum_q J_q; min_jacobian, m = +inf and then per frame
//                 and point m = (J_q < m) ? J_q : m, so a NaN never replaces m.  Nothing is clamped: J_q = 0 gives inf or NaN,
//                 a negative J_q is carried through.  256 VGPRs and 22 AGPRs, no scratch, one wave per SIMD (fsi_rate.hpp).
//
// No LDS, no atomics, FP64 vector loads and stores.  Floating-point contraction is off, as in fsi_band.hip and fsi_phase.hip:
// the NumPy twins (hi_pass.cell_rate, hi_pass.cell_rate_current) round every product and every sum, and the device equals them bit for bit.
#include "fsi_rate.hpp"
#include "fsi_cell.hpp"

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
  double q = 0.0, T[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[i][j] = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    fence_cell_gradients(gl);
    double G[3][3];
    vertex_gradient_of(w, gl, t, G);
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
  CellLane lane;
  load_cell_lane(conn, gl_all, c, lane);
  double s = 0.0;
  for (int64_t k = 0; k < count; ++k) {
    double w[10][3];
    gather_cell_frame(x + k * frame_stride, lane, w);
    s = s + cell_rate_of(w, lane.gl);
  }
  out[c] = s / (double)count;
}

// the sum of the four vertex gradients, in vertex order from +0.0
__device__ __forceinline__ void vertex_sum_of(const double (&G)[4][3][3], double (&T)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int t = 0; t < 4; ++t) s = s + G[t][i][j];
      T[i][j] = s;
    }
}

// One frame of one cell in the current configuration: G, D the vertex gradients of the field and of the displacement.  r: the
// mean of 2 S:S over the deformed cell; vol: 0.25 sum_q J_q; m: the running minimum of J_q.  Every operation in the order of
// hi_pass.cell_rate_current.
__device__ __forceinline__ void current_rate_of(const double (&G)[4][3][3], const double (&D)[4][3][3], double& r, double& vol, double& m) {
  const double QA = 0.5854101966249685, QB = 0.1381966011250105, QAB = QA - QB;
  double TG[3][3], TD[3][3];
  vertex_sum_of(G, TG);
  vertex_sum_of(D, TD);
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double g[3][3], F[3][3], A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        g[i][j] = QB * TG[i][j] + QAB * G[q][i][j];
        const double d = QB * TD[i][j] + QAB * D[q][i][j];
        F[i][j] = i == j ? 1.0 + d : d;
      }
    A[0][0] = F[1][1] * F[2][2] - F[1][2] * F[2][1];      // adj F, the transposed cofactors
    A[0][1] = F[0][2] * F[2][1] - F[0][1] * F[2][2];
    A[0][2] = F[0][1] * F[1][2] - F[0][2] * F[1][1];
    A[1][0] = F[1][2] * F[2][0] - F[1][0] * F[2][2];
    A[1][1] = F[0][0] * F[2][2] - F[0][2] * F[2][0];
    A[1][2] = F[0][2] * F[1][0] - F[0][0] * F[1][2];
    A[2][0] = F[1][0] * F[2][1] - F[1][1] * F[2][0];
    A[2][1] = F[0][1] * F[2][0] - F[0][0] * F[2][1];
    A[2][2] = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    const double J = (F[0][0] * A[0][0] + F[0][1] * A[1][0]) + F[0][2] * A[2][0];
    double L[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) L[i][j] = ((g[i][0] * A[0][j] + g[i][1] * A[1][j]) + g[i][2] * A[2][j]) / J;
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double S = 0.5 * (L[i][j] + L[j][i]);
        e = e + S * S;
      }
    num = num + J * (2.0 * e);
    den = den + J;
    m = J < m ? J : m;
  }
  r = num / den;
  vol = 0.25 * den;
}

__global__ __launch_bounds__(256) void k_cell_rate_current(int64_t n, const int32_t* __restrict__ conn, const double* __restrict__ gl_all,
                                                           const double* __restrict__ x, int64_t frame_stride,
                                                           const double* __restrict__ geo, int64_t geo_stride, int64_t count,
                                                           double* __restrict__ rate, double* __restrict__ volume_ratio,
                                                           double* __restrict__ min_jacobian) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  CellLane lane;
  load_cell_lane(conn, gl_all, c, lane);
  double s = 0.0, sv = 0.0, m = __builtin_inf();
  for (int64_t k = 0; k < count; ++k) {
    // the displacement's ten triples become its vertex gradients before the field's are needed: thirty nodal values and
    // seventy-two gradient entries are live at most, not the sixty nodal values of both
    double w[10][3], D[4][3][3], G[4][3][3];
    gather_cell_frame(geo + k * geo_stride, lane, w);
    vertex_gradients_of(w, lane.gl, D);
    gather_cell_frame(x + k * frame_stride, lane, w);
    vertex_gradients_of(w, lane.gl, G);
    double r, vol;
    current_rate_of(G, D, r, vol, m);
    s = s + r;
    sv = sv + vol;
  }
  rate[c] = s / (double)count;
  volume_ratio[c] = sv / (double)count;
  min_jacobian[c] = m;
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

void launch_cell_rate_current(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                              const double* geo, int64_t geo_stride, int64_t count, double* rate, double* volume_ratio,
                              double* min_jacobian) {
  if (n > 0 && count > 0)
    hipLaunchKernelGGL(k_cell_rate_current, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, conn, gl, x, frame_stride, geo,
                       geo_stride, count, rate, volume_ratio, min_jacobian);
}

}  // namespace fsi
