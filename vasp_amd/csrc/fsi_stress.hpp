// Solid stress / strain of one cell: the per-cell arithmetic of k_stress_strain (fsi_post.hip), shared with the sample kernel
// of the stress / strain session (fsi_stress.hip) so that both produce the same bits.
#pragma once
#include "fsi_kernels.hpp"

namespace fsi {

namespace {

// Keast-24 tables as in fsi_assembly.hip: every translation unit that includes this header keeps its own constant copies
// (upload_post_tables fills those of fsi_post.hip, upload_stress_tables those of fsi_stress.hip)
__constant__ double p_qw[NQ];
__constant__ double p_dN[NQ][10][3];
__constant__ double p_L[NQ][4];

__device__ inline double max_eig_sym3(const double T[3][3]) {
  // largest root of the characteristic polynomial, trigonometric form (Kopp 2008, eqs. 21-34) with the perturbations of
  // turtleFSI's get_eig so that p, q and the discriminant never vanish
  const double I1 = T[0][0] + T[1][1] + T[2][2];
  double TT = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) TT += T[i][j] * T[i][j];
  const double I2 = 0.5 * (I1 * I1 - TT);
  const double I3 = T[0][0] * (T[1][1] * T[2][2] - T[1][2] * T[2][1]) - T[0][1] * (T[1][0] * T[2][2] - T[1][2] * T[2][0]) +
                    T[0][2] * (T[1][0] * T[2][1] - T[1][1] * T[2][0]);
  double p = I1 * I1 - 3.0 * I2;
  if (p < 1e-16) p = fabs(p) + 2e-16;
  double q = 13.5 * I3 + I1 * I1 * I1 - 4.5 * I1 * I2;
  if (fabs(q) < 1e-24) q = q + (q > 0.0 ? 2e-24 : (q < 0.0 ? -2e-24 : 0.0));
  double nom2 = 27.0 * (0.25 * I2 * I2 * (p - I2) + I3 * (6.75 * I3 - q));
  if (nom2 < 1e-40) nom2 = fabs(nom2) + 2e-40;
  const double phi = atan2(sqrt(nom2), q) / 3.0;
  return (sqrt(p) * 2.0 * cos(phi) + I1) / 3.0;
}

// compute_stress_strain [REF src/vasp/postprocessing/postprocessing_fenics/compute_stress_strain.py:188-263] on solid cell c,
// run by one 64-lane workgroup (lanes = quadrature points, LDS for the projections).  oc[80]: TrueStress [4][9],
// GreenLagrangeStrain [4][9], MaxPrincipalStress [4], MaxPrincipalStrain [4] (DG1 coefficient a = local vertex a).
// Returns on lanes 0..7 the principal value the lane wrote to oc[72 + lane], 0 on the others.  PRINCIPAL false: the two
// tensors only (oc[0 .. 72), the same instructions up to there), for a caller that keeps no principal values.
template <bool PRINCIPAL = true>
__device__ inline double stress_strain_cell(const ElemArrays& ea, const ElemParams& ep, const double* __restrict__ U, int64_t c,
                                           double* __restrict__ oc) {
  const int lane = threadIdx.x;
  __shared__ double sD[30], sJ[10];
  __shared__ double sF[NQ][18];          // sigma(9), E(9) at the quadrature points, weighted
  __shared__ double sX[72];              // DG1 coefficients of the two tensors
  __shared__ double sP[NQ][2];           // principal values at the quadrature points, weighted
  if (lane < 30) sD[lane] = U[ea.cell_dofs[c * NLOC + lane]];
  if (lane < 10) sJ[lane] = ea.geom[c * 10 + lane];
  __syncthreads();
  const SolidProps sp = ep.solid[ea.cell_region[c]];
  if (lane < NQ) {
    double g[3][3] = {};
    for (int a = 0; a < 10; ++a) {
      const double r0 = p_dN[lane][a][0], r1 = p_dN[lane][a][1], r2 = p_dN[lane][a][2];
      double G[3];
      for (int j = 0; j < 3; ++j) G[j] = r0 * sJ[j] + r1 * sJ[3 + j] + r2 * sJ[6 + j];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) g[i][j] += sD[i * 10 + a] * G[j];
    }
    double P[3][3], Fi[3][3];
    piola<double>(sp, g, P);                              // P = F S
    const double J = inv_det_F<double>(g, Fi);
    const double w = sJ[9] * p_qw[lane];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0.0, cij = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double Fjk = g[j][k] + (j == k ? 1.0 : 0.0);
          s += P[i][k] * Fjk;                             // (F S) F^T
          cij += (g[k][i] + (k == i ? 1.0 : 0.0)) * (g[k][j] + (k == j ? 1.0 : 0.0));
        }
        sF[lane][3 * i + j] = w * s / J;
        sF[lane][9 + 3 * i + j] = w * 0.5 * (cij - (i == j ? 1.0 : 0.0));
      }
  }
  __syncthreads();
  // rhs_a = sum_q L[q][a] f_q ; the P1 mass matrix of a tetrahedron is vol/20 (I + 1 1^T), its inverse 20/vol (I - 1 1^T / 5)
  const double vol = sJ[9] / 6.0;
  for (int o = lane; o < 72; o += 64) {
    const int a = o / 18, comp = o % 18;
    double s = 0.0;
    for (int q = 0; q < NQ; ++q) s += p_L[q][a] * sF[q][comp];
    sX[o] = s;
  }
  __syncthreads();
  double keep[2] = {0.0, 0.0};
  for (int o = lane, k = 0; o < 72; o += 64, ++k) {
    const int comp = o % 18;
    const double tot = sX[comp] + sX[18 + comp] + sX[36 + comp] + sX[54 + comp];
    keep[k] = (20.0 / vol) * (sX[o] - 0.2 * tot);
  }
  __syncthreads();
  for (int o = lane, k = 0; o < 72; o += 64, ++k) sX[o] = keep[k];
  __syncthreads();
  for (int o = lane; o < 72; o += 64) {
    const int a = o / 18, comp = o % 18;
    oc[(comp < 9 ? 0 : 36) + a * 9 + (comp % 9)] = sX[o];
  }
  if (!PRINCIPAL) return 0.0;
  if (lane < NQ) {
    const double w = sJ[9] * p_qw[lane];
    for (int t = 0; t < 2; ++t) {
      double T[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double s = 0.0;
          for (int a = 0; a < 4; ++a) s += p_L[lane][a] * sX[a * 18 + 9 * t + 3 * i + j];
          T[i][j] = s;
        }
      for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) T[i][j] = T[j][i] = 0.5 * (T[i][j] + T[j][i]);
      sP[lane][t] = w * max_eig_sym3(T);
    }
  }
  __syncthreads();
  double pv = 0.0;
  if (lane < 8) {
    const int t = lane / 4, a = lane % 4;
    double r[4];
    for (int b = 0; b < 4; ++b) {
      double s = 0.0;
      for (int q = 0; q < NQ; ++q) s += p_L[q][b] * sP[q][t];
      r[b] = s;
    }
    pv = (20.0 / vol) * (r[a] - 0.2 * (r[0] + r[1] + r[2] + r[3]));
    oc[72 + 4 * t + a] = pv;
  }
  return pv;
}

}  // namespace

}  // namespace fsi
