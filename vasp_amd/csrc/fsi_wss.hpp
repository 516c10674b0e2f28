// DG1-projected tangential traction of one boundary cell: the per-cell arithmetic of k_wss (fsi_post.hip), shared with the
// hemodynamics sample kernel (fsi_hemo.hip) so that both produce the same bits.
#pragma once
#include "fsi_kernels.hpp"

namespace fsi {

// Stress of compute_hemodynamics [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:91-157] on
// cell c: Ft = F - (F.n) n with F = -2 mu sym(grad u) n on the exterior facets set in `mask` (bit f: the facet opposite
// local vertex f), projected with the surface mass matrix onto the DG1 space of the cell (zero rows -> identity).
// b[a][i]: coefficient of local vertex a, component i (0 on vertices that touch no exterior facet).  Undeformed geometry.
__device__ inline void wss_dg1_cell(const ElemArrays& ea, const double* __restrict__ U, int64_t c, int mask, double mu,
                                    double b[4][3]) {
  const double* Jg = ea.geom + c * 10;
  double gl[4][3];                                  // physical gradients of the barycentric coordinates
  for (int j = 0; j < 3; ++j) {
    gl[1][j] = Jg[j]; gl[2][j] = Jg[3 + j]; gl[3][j] = Jg[6 + j];
    gl[0][j] = -(Jg[j] + Jg[3 + j] + Jg[6 + j]);
  }
  const double vol = Jg[9] / 6.0;
  double v[10][3];
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 10; ++a) v[a][i] = U[ea.cell_dofs[c * NLOC + 30 + i * 10 + a]];
  const int E[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
  // grad v is linear on the cell: its values at the four vertices
  double gv[4][3][3];
  for (int vtx = 0; vtx < 4; ++vtx)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int a = 0; a < 4; ++a) s += v[a][i] * ((a == vtx ? 3.0 : -1.0) * gl[a][j]);
        for (int e = 0; e < 6; ++e) {
          const int p = E[e][0], q = E[e][1];
          s += v[4 + e][i] * 4.0 * ((p == vtx ? 1.0 : 0.0) * gl[q][j] + (q == vtx ? 1.0 : 0.0) * gl[p][j]);
        }
        gv[vtx][i][j] = s;
      }
  double M[4][4] = {};
  for (int a = 0; a < 4; ++a)
    for (int i = 0; i < 3; ++i) b[a][i] = 0.0;
  for (int f = 0; f < 4; ++f) {
    if (!(mask & (1 << f))) continue;
    const double gn = sqrt(gl[f][0] * gl[f][0] + gl[f][1] * gl[f][1] + gl[f][2] * gl[f][2]);
    const double n[3] = {-gl[f][0] / gn, -gl[f][1] / gn, -gl[f][2] / gn};       // outward: away from the opposite vertex
    const double area = 3.0 * vol * gn;
    double Ft[4][3];
    for (int vtx = 0; vtx < 4; ++vtx) {
      if (vtx == f) continue;
      double Fv[3], Fn = 0.0;
      for (int i = 0; i < 3; ++i) {
        double s = 0.0;
        for (int j = 0; j < 3; ++j) s += mu * (gv[vtx][i][j] + gv[vtx][j][i]) * n[j];
        Fv[i] = -s;
        Fn += Fv[i] * n[i];
      }
      for (int i = 0; i < 3; ++i) Ft[vtx][i] = Fv[i] - Fn * n[i];
    }
    for (int a = 0; a < 4; ++a) {
      if (a == f) continue;
      for (int bb = 0; bb < 4; ++bb) {
        if (bb == f) continue;
        const double m = area / 12.0 * (a == bb ? 2.0 : 1.0);      // facet mass matrix of the P1 traces
        M[a][bb] += m;
        for (int i = 0; i < 3; ++i) b[a][i] += m * Ft[bb][i];
      }
    }
  }
  for (int a = 0; a < 4; ++a) {
    double s = 0.0;
    for (int bb = 0; bb < 4; ++bb) s += fabs(M[a][bb]);
    if (s == 0.0) M[a][a] = 1.0;                                    // ident_zeros of the surface mass matrix
  }
  // Gaussian elimination (symmetric positive definite after the identity rows)
  for (int k = 0; k < 4; ++k) {
    const double piv = 1.0 / M[k][k];
    for (int r = k + 1; r < 4; ++r) {
      const double l = M[r][k] * piv;
      if (l == 0.0) continue;
      for (int cc = k; cc < 4; ++cc) M[r][cc] -= l * M[k][cc];
      for (int i = 0; i < 3; ++i) b[r][i] -= l * b[k][i];
    }
  }
  for (int k = 3; k >= 0; --k)
    for (int i = 0; i < 3; ++i) {
      double s = b[k][i];
      for (int cc = k + 1; cc < 4; ++cc) s -= M[k][cc] * b[cc][i];
      b[k][i] = s / M[k][k];
    }
}

}  // namespace fsi
