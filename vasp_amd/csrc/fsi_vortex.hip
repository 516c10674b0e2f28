// Vortex identification on a recorded velocity history, on the device: the Q-criterion, enstrophy, helicity and kinetic energy
// of every listed cell (vasp_amd/vortex.py), and their ordered weighted sums over the cells.
//
// Replaces nothing in the reference.  The history is that of a band-pass session (hist[frame][row], a node's three components
// contiguous), the cell list and its gradients those of fsi_band_cells (fsi_rate.hip).
//
//   k_cell_vortex : one lane per listed cell, the geometry of k_cell_rate.  The lane keeps the cell's ten node indices and its
//                 twelve gradient values in registers and walks `count` frames of one series.  Per frame it gathers the ten
//                 nodes' triples w (240 B) and forms G_t = grad w at the four vertices t by vertex_gradient_of (fsi_cell.hpp,
//                 with the lane state and the gather), one vertex after the other.  The gradient of a P2 field is linear on the
//                 cell, so the cell mean of a product of two linear f, h is 0.05 (sum_t f_t h_t + (sum_t f_t)(sum_t h_t)), and
//                 with omega_t = (G_t[2][1] - G_t[1][2], G_t[0][2] - G_t[2][0], G_t[1][0] - G_t[0][1]), T = sum_t G_t:
//                   field 0  Q            -0.5 * (0.05 * (sum_t sum_ij G_t[i][j] G_t[j][i] + sum_ij T[i][j] T[j][i]))
//                   field 1  enstrophy    0.05 * (sum_t |omega_t|^2 + |W|^2), W = (T[2][1] - T[1][2], T[0][2] - T[2][0], T[1][0] - T[0][1])
//                   field 2  helicity     sum_t sum_i (sum_a M[a][t] w[a][i]) omega_t[i], M the mean of P2 basis a times L_t
//                   field 3  abs_helicity |field 2| of the frame: the absolute value of the cell mean, not the mean of |w . omega|
//                   field 4  speed2       sum_i sum_a w[a][i] (sum_b MM[a][b] w[b][i]), MM the P2 mass matrix over |K|
//                 Each vertex's omega_t goes into the helicity sum before the next vertex begins, so one G_t is live beside w.
//                 out[f][c] = (((+0.0 + r_0) + r_1) + ...) / count per field: the sum in frame order, a true division; one
//                 frame gives its own bits.  NaN and inf propagate, nothing is clamped.  No LDS, no atomics.
//
//   k_cell_wsum : partial[f][b] of workgroup b, the sum of weight[c] * value[f][c] over its 256 consecutive cells in a fixed
//                 bracket: p_c = weight_c * value_c (one rounding; lanes past n hold +0.0); in a wave a butterfly with xor
//                 strides 1, 2, 4, 8, 16, 32 - a balanced tree over adjacent pairs, every lane ends with the same bits, the
//                 addition being commutative -; the four wave sums through LDS, ((s0 + s1) + s2) + s3.
//   k_cell_wsum_close : one workgroup; lane f < 5 adds field f's partials from +0.0 in ascending workgroup order (one chain of
//                 additions; the loop is unrolled so that sixteen loads are in flight ahead of it).
//
// FP64 vector loads and stores only.  Floating-point contraction is off: the NumPy twins (hi_pass.cell_vortex, hi_pass.cell_wsum)
// round every product and every sum, and the device equals them bit for bit.
#include "fsi_vortex.hpp"
#include "fsi_cell.hpp"

#pragma clang fp contract(off)

namespace fsi {

namespace {

// 60 M[a][t]: the mean over the cell of P2 basis function a times barycentric coordinate t.  Vertex a: 0 at t == a, else -1;
// edge {p, r}: 4 at t in {p, r}, else 2.  420 MM[a][b]: the P2 mass matrix over |K|.  Vertex-vertex 6 / 1; vertex-edge -4 if
// the vertex is an end of the edge, else -6; edge-edge 32 / 16 sharing a vertex / 8 opposite.  (hi_pass.VORTEX_M, VORTEX_MM)
__device__ constexpr int m60(int a, int t) {
  return a < 4 ? (a == t ? 0 : -1) : ((kEdge[a - 4][0] == t || kEdge[a - 4][1] == t) ? 4 : 2);
}

__device__ constexpr int mm420(int a, int b) {
  if (a < 4 && b < 4) return a == b ? 6 : 1;
  if (a < 4) return (kEdge[b - 4][0] == a || kEdge[b - 4][1] == a) ? -4 : -6;
  if (b < 4) return mm420(b, a);
  if (a == b) return 32;
  const int p = kEdge[a - 4][0], r = kEdge[a - 4][1], s = kEdge[b - 4][0], u = kEdge[b - 4][1];
  return (p == s || p == u || r == s || r == u) ? 16 : 8;
}

// The five values of one frame of one cell.  Every operation in the order of hi_pass.cell_vortex.
__device__ __forceinline__ void cell_vortex_of(const double (&w)[10][3], double (&gl)[4][3], double (&r)[FSI_VORTEX_FIELDS]) {
  double qd = 0.0, ed = 0.0, h = 0.0, T[3][3];
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
        qd = qd + G[i][j] * G[j][i];
        T[i][j] = T[i][j] + G[i][j];
      }
    const double om[3] = {G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]};
#pragma unroll
    for (int i = 0; i < 3; ++i) ed = ed + om[i] * om[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double u = 0.0;
#pragma unroll
      for (int a = 0; a < 10; ++a) u = u + ((double)m60(a, t) / 60.0) * w[a][i];
      h = h + u * om[i];
    }
    // this vertex is done before the next begins
    asm volatile("" : "+v"(qd), "+v"(ed), "+v"(h));
  }
  double qp = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) qp = qp + T[i][j] * T[j][i];
  const double W[3] = {T[2][1] - T[1][2], T[0][2] - T[2][0], T[1][0] - T[0][1]};
  double ep = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) ep = ep + W[i] * W[i];
  double s2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int a = 0; a < 10; ++a) {
      double u = 0.0;
#pragma unroll
      for (int b = 0; b < 10; ++b) u = u + ((double)mm420(a, b) / 420.0) * w[b][i];
      s2 = s2 + w[a][i] * u;
    }
  r[FSI_VORTEX_Q] = -0.5 * (0.05 * (qd + qp));
  r[FSI_VORTEX_ENSTROPHY] = 0.05 * (ed + ep);
  r[FSI_VORTEX_HELICITY] = h;
  r[FSI_VORTEX_ABS_HELICITY] = __builtin_fabs(h);
  r[FSI_VORTEX_SPEED2] = s2;
}

__global__ __launch_bounds__(256) void k_cell_vortex(int64_t n, const int32_t* __restrict__ conn, const double* __restrict__ gl_all,
                                                     const double* __restrict__ x, int64_t frame_stride, int64_t count,
                                                     double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  CellLane lane;
  load_cell_lane(conn, gl_all, c, lane);
  double s[FSI_VORTEX_FIELDS];
#pragma unroll
  for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) s[f] = 0.0;
  for (int64_t k = 0; k < count; ++k) {
    double w[10][3], r[FSI_VORTEX_FIELDS];
    gather_cell_frame(x + k * frame_stride, lane, w);
    cell_vortex_of(w, lane.gl, r);
#pragma unroll
    for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) s[f] = s[f] + r[f];
  }
#pragma unroll
  for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) out[(int64_t)f * n + c] = s[f] / (double)count;
}

__global__ __launch_bounds__(256) void k_cell_wsum(int64_t n, const double* __restrict__ weight, const double* __restrict__ value,
                                                   int64_t nblock, double* __restrict__ partial) {
  __shared__ double wave_sum[4];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double wc = c < n ? weight[c] : 0.0;
  for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) {
    double p = 0.0;
    if (c < n) p = wc * value[(int64_t)f * n + c];
#pragma unroll
    for (int stride = 1; stride < 64; stride <<= 1) p = p + __shfl_xor(p, stride, 64);
    if (lane == 0) wave_sum[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)f * nblock + blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_cell_wsum_close(int64_t nblock, const double* __restrict__ partial, double* __restrict__ sums) {
  const int f = threadIdx.x;
  if (f >= FSI_VORTEX_FIELDS) return;
  double s = 0.0;
  // the additions are one chain; unrolled, the loads of sixteen partials are in flight ahead of it
#pragma unroll 16
  for (int64_t b = 0; b < nblock; ++b) s = s + partial[(int64_t)f * nblock + b];
  sums[f] = s;
}

}  // namespace

void launch_cell_vortex(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                        int64_t count, double* out) {
  if (n > 0 && count > 0)
    hipLaunchKernelGGL(k_cell_vortex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, conn, gl, x, frame_stride, count, out);
}

void launch_cell_wsum(hipStream_t st, int64_t n, const double* weight, const double* value, double* partial, double* sums) {
  if (n <= 0) return;
  const int64_t nblock = cell_wsum_blocks(n);
  hipLaunchKernelGGL(k_cell_wsum, dim3((unsigned)nblock), dim3(256), 0, st, n, weight, value, nblock, partial);
  hipLaunchKernelGGL(k_cell_wsum_close, dim3(1), dim3(64), 0, st, nblock, partial, sums);
}

}  // namespace fsi
