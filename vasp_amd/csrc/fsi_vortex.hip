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
//   k_cell_vortex_current : the same in the current configuration x = X + d(X) of an ALE run, the geometry of
//                 k_cell_rate_current: one lane per listed cell walks `count` frames of a field w and of the displacement d
//                 together (480 B gathered per cell and frame).  The displacement's ten triples become its four vertex
//                 gradients D_t, then the field's its G_t (vertex_gradients_of, fsi_cell.hpp); w stays live for the point
//                 values.  The rule is the 14-point positive interior rule of degree 5 (helicity is of degree 3, |v|^2 of
//                 degree 4, det F cubic), weights summing to 1, in barycentric coordinates
//                   p = 0..3   1 - 3 a1 on vertex p, a1 = 0.31088591926330060980 on the others     om = 0.11268792571801585080
//                   p = 4..7   1 - 3 a2 on vertex p - 4, a2 = 0.092735250310891226402 on the others om = 0.073493043116361949544
//                   p = 8..13  0.5 - b on the ends of local edge p - 8, b = 0.045503704125649649492
//                              on the other two                                                    om = 0.042546020777081466438
//                 kept with the P2 basis values at its points as one table of compile-time constants (kRule) that the point
//                 loop, which is not unrolled, reads through scalar loads.  Per point p: G_p = ((lam_0 G_0 + lam_1 G_1) +
//                 lam_2 G_2) + lam_3 G_3 and D_p likewise - exact, the gradients being linear on the cell -, F_p = I + D_p,
//                 A_p = adj F_p, J_p = det F_p, L_p = (G_p A_p) * (1 / J_p), v_p = sum_a N_a(lam_p) w[a],
//                 omega_p = (L[2][1] - L[1][2], L[0][2] - L[2][0], L[1][0] - L[0][1]) and the integrands
//                   f_0 = -0.5 sum_ij L_ij L_ji   f_1 = |omega_p|^2   f_2 = v_p . omega_p   f_4 = |v_p|^2.
//                 Per frame Jbar = sum_p om_p J_p, the deformed cell's volume over the undeformed (exact for a P2 d), the
//                 numerators n_f = sum_p (om_p J_p) f_p, n_3 = |n_2|, and the means over the deformed cell r_f = n_f / Jbar,
//                 r_3 = |r_2|.  out[12][n]: rows 0..5 the means over the frames of r_0..r_4 and Jbar, rows 6..11 those of
//                 n_0..n_4 and Jbar again, each the sum from +0.0 in frame order and a true division by count.  Nothing is
//                 clamped: J_p = 0 gives inf or NaN, a negative J_p is carried through.  With d = 0 every integrand is of
//                 degree <= 4 on the cell, the rule exact and r_f is field f of k_cell_vortex to rounding.  256 VGPRs and 80 AGPRs,
//                 no scratch, one wave per SIMD (fsi_vortex.hpp).
//
//   k_cell_wsum : partial[f][b] of workgroup b, the sum of weight[c] * value[f][c] over its 256 consecutive cells in a fixed
//                 bracket: p_c = weight_c * value_c (one rounding; lanes past n hold +0.0); in a wave a butterfly with xor
//                 strides 1, 2, 4, 8, 16, 32 - a balanced tree over adjacent pairs, every lane ends with the same bits, the
//                 addition being commutative -; the four wave sums through LDS, ((s0 + s1) + s2) + s3.
//   k_cell_wsum_close : one workgroup; lane f < nfield adds field f's partials from +0.0 in ascending workgroup order (one chain of
//                 additions; the loop is unrolled so that sixteen loads are in flight ahead of it).
//
// FP64 vector loads and stores only.  Floating-point contraction is off: the NumPy twins (hi_pass.cell_vortex,
// hi_pass.cell_vortex_current, hi_pass.cell_wsum) round every product and every sum, and the device equals them bit for bit.
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

// The 14-point rule of degree 5 and the P2 basis at its points (hi_pass.VORTEX_RULE_*): per point the four barycentrics, the
// weight and the ten basis values N_a = lam_a (2 lam_a - 1) at a vertex, (4 lam_r) lam_s on the edge {r, s}.  Every entry is
// formed at compile time by the operations the twin forms it with.
constexpr double kRuleA1 = 0.31088591926330060980, kRuleW1 = 0.11268792571801585080;
constexpr double kRuleA2 = 0.092735250310891226402, kRuleW2 = 0.073493043116361949544;
constexpr double kRuleB = 0.045503704125649649492, kRuleW3 = 0.042546020777081466438;
constexpr int kRulePoints = 14;

constexpr double rule_lam(int p, int t) {
  if (p < 4) return t == p ? 1.0 - 3.0 * kRuleA1 : kRuleA1;
  if (p < 8) return t == p - 4 ? 1.0 - 3.0 * kRuleA2 : kRuleA2;
  return (kEdge[p - 8][0] == t || kEdge[p - 8][1] == t) ? 0.5 - kRuleB : kRuleB;
}

struct RuleTable {
  double lam[kRulePoints][4], om[kRulePoints], basis[kRulePoints][10];
  constexpr RuleTable() : lam{}, om{}, basis{} {
    for (int p = 0; p < kRulePoints; ++p) {
      for (int t = 0; t < 4; ++t) lam[p][t] = rule_lam(p, t);
      om[p] = p < 4 ? kRuleW1 : p < 8 ? kRuleW2 : kRuleW3;
      for (int a = 0; a < 4; ++a) basis[p][a] = lam[p][a] * (2.0 * lam[p][a] - 1.0);
      for (int e = 0; e < 6; ++e) basis[p][4 + e] = (4.0 * lam[p][kEdge[e][0]]) * lam[p][kEdge[e][1]];
    }
  }
};
__constant__ constexpr RuleTable kRule{};

// One frame of one cell in the current configuration: w the field's nodal values, G and D the vertex gradients of the field and
// of the displacement.  n[0..4]: the numerators; jbar: the volume ratio.  Every operation in the order of
// hi_pass.cell_vortex_current.
__device__ __forceinline__ void current_vortex_of(const double (&w)[10][3], const double (&G)[4][3][3], const double (&D)[4][3][3],
                                                  double (&n)[FSI_VORTEX_FIELDS], double& jbar) {
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, n4 = 0.0, jb = 0.0;
  // not unrolled: one point's temporaries beside the frame's 102 values, and the rule read as scalars
#pragma unroll 1
  for (int p = 0; p < kRulePoints; ++p) {
    const double l0 = kRule.lam[p][0], l1 = kRule.lam[p][1], l2 = kRule.lam[p][2], l3 = kRule.lam[p][3];
    double g[3][3], F[3][3], A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        g[i][j] = ((l0 * G[0][i][j] + l1 * G[1][i][j]) + l2 * G[2][i][j]) + l3 * G[3][i][j];
        const double d = ((l0 * D[0][i][j] + l1 * D[1][i][j]) + l2 * D[2][i][j]) + l3 * D[3][i][j];
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
    const double rJ = 1.0 / J;
    double L[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) L[i][j] = ((g[i][0] * A[0][j] + g[i][1] * A[1][j]) + g[i][2] * A[2][j]) * rJ;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) q = q + L[i][j] * L[j][i];
    const double om[3] = {L[2][1] - L[1][2], L[0][2] - L[2][0], L[1][0] - L[0][1]};
    double e = 0.0, h = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) e = e + om[i] * om[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < 10; ++a) v = v + kRule.basis[p][a] * w[a][i];
      h = h + v * om[i];
      s2 = s2 + v * v;
    }
    const double wj = kRule.om[p] * J;
    jb = jb + wj;
    n0 = n0 + wj * (-0.5 * q);
    n1 = n1 + wj * e;
    n2 = n2 + wj * h;
    n4 = n4 + wj * s2;
  }
  n[FSI_VORTEX_Q] = n0;
  n[FSI_VORTEX_ENSTROPHY] = n1;
  n[FSI_VORTEX_HELICITY] = n2;
  n[FSI_VORTEX_ABS_HELICITY] = __builtin_fabs(n2);
  n[FSI_VORTEX_SPEED2] = n4;
  jbar = jb;
}

__global__ __launch_bounds__(256) void k_cell_vortex_current(int64_t n, const int32_t* __restrict__ conn, const double* __restrict__ gl_all,
                                                             const double* __restrict__ x, int64_t frame_stride,
                                                             const double* __restrict__ geo, int64_t geo_stride, int64_t count,
                                                             double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  CellLane lane;
  load_cell_lane(conn, gl_all, c, lane);
  double sr[FSI_VORTEX_FIELDS], sn[FSI_VORTEX_FIELDS], sj = 0.0;
#pragma unroll
  for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) sr[f] = sn[f] = 0.0;
  for (int64_t k = 0; k < count; ++k) {
    // the displacement's ten triples become its vertex gradients before the field's are gathered, as in k_cell_rate_current;
    // the field's thirty nodal values stay beside the seventy-two gradient entries for the point values
    double w[10][3], D[4][3][3], G[4][3][3], nf[FSI_VORTEX_FIELDS], jbar;
    gather_cell_frame(geo + k * geo_stride, lane, w);
    vertex_gradients_of(w, lane.gl, D);
    gather_cell_frame(x + k * frame_stride, lane, w);
    vertex_gradients_of(w, lane.gl, G);
    current_vortex_of(w, G, D, nf, jbar);
#pragma unroll
    for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) {
      if (f == FSI_VORTEX_ABS_HELICITY) continue;
      sr[f] = sr[f] + nf[f] / jbar;
      sn[f] = sn[f] + nf[f];
    }
    sr[FSI_VORTEX_ABS_HELICITY] = sr[FSI_VORTEX_ABS_HELICITY] + __builtin_fabs(nf[FSI_VORTEX_HELICITY] / jbar);
    sn[FSI_VORTEX_ABS_HELICITY] = sn[FSI_VORTEX_ABS_HELICITY] + nf[FSI_VORTEX_ABS_HELICITY];
    sj = sj + jbar;
  }
  const double cnt = (double)count, vr = sj / cnt;
#pragma unroll
  for (int f = 0; f < FSI_VORTEX_FIELDS; ++f) {
    out[(int64_t)f * n + c] = sr[f] / cnt;
    out[(int64_t)(FSI_VORTEX_CURRENT_FIELDS + f) * n + c] = sn[f] / cnt;
  }
  out[(int64_t)FSI_VORTEX_VOLUME_RATIO * n + c] = vr;
  out[(int64_t)(FSI_VORTEX_CURRENT_FIELDS + FSI_VORTEX_VOLUME_RATIO) * n + c] = vr;
}

__global__ __launch_bounds__(256) void k_cell_wsum(int64_t n, int nfield, const double* __restrict__ weight,
                                                   const double* __restrict__ value, int64_t nblock, double* __restrict__ partial) {
  __shared__ double wave_sum[4];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double wc = c < n ? weight[c] : 0.0;
  for (int f = 0; f < nfield; ++f) {
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

__global__ __launch_bounds__(64) void k_cell_wsum_close(int nfield, int64_t nblock, const double* __restrict__ partial,
                                                        double* __restrict__ sums) {
  const int f = threadIdx.x;
  if (f >= nfield) return;
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

void launch_cell_vortex_current(hipStream_t st, int64_t n, const int32_t* conn, const double* gl, const double* x, int64_t frame_stride,
                                const double* geo, int64_t geo_stride, int64_t count, double* out) {
  if (n > 0 && count > 0)
    hipLaunchKernelGGL(k_cell_vortex_current, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, conn, gl, x, frame_stride, geo,
                       geo_stride, count, out);
}

void launch_cell_wsum(hipStream_t st, int64_t n, int nfield, const double* weight, const double* value, double* partial, double* sums) {
  if (n <= 0 || nfield < 1 || nfield > 64) return;
  const int64_t nblock = cell_wsum_blocks(n);
  hipLaunchKernelGGL(k_cell_wsum, dim3((unsigned)nblock), dim3(256), 0, st, n, nfield, weight, value, nblock, partial);
  hipLaunchKernelGGL(k_cell_wsum_close, dim3(1), dim3(64), 0, st, nfield, nblock, partial, sums);
}

}  // namespace fsi
