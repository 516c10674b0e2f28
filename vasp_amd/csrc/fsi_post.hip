// Solid stress / strain and wall shear stress from the resident state.
//
// Replaces, per saved time step, the element loops of VaSP's FEniCS post-processing:
//   k_stress_strain : compute_stress_strain [REF src/vasp/postprocessing/postprocessing_fenics/compute_stress_strain.py:188-263]
//                     Cauchy stress 1/J F S F^T and Green-Lagrange strain E of the P2 displacement, L2-projected onto
//                     tensor DG1 cell by cell (solve_dg), then the largest principal value of each projected tensor
//                     (common.get_eig) projected onto scalar DG1 (project_dg).  The constitutive routines are those of
//                     the residual kernels (fsi_element.hpp); the per-cell body is stress_strain_cell (fsi_stress.hpp),
//                     which the stress / strain session's k_stress_sample (fsi_stress.hip) shares.
//   k_wss           : Stress of compute_hemodynamics [REF .../compute_hemodynamics.py:91-157]: Ft = F - (F.n) n with
//                     F = -2 mu sym(grad u) n on exterior facets, projected with the surface mass matrix onto the DG1
//                     space of the boundary cell (zero rows -> identity).
// Both are cell-local: one wavefront per solid cell (lanes = quadrature points, LDS for the projections), one lane per
// boundary cell.  Output is DG1 coefficients (one per local vertex), the layout the reference's write_checkpoint files
// carry through cell_dofs.  HBM traffic per solid cell: 30 gathered doubles + 80 geometry bytes in, 80 doubles out.
#include "fsi_kernels.hpp"
#include "fsi_stress.hpp"
#include "fsi_wss.hpp"

namespace fsi {

namespace {

bool p_tables_ready = false;

// out[c][80]: TrueStress [4][9], GreenLagrangeStrain [4][9], MaxPrincipalStress [4], MaxPrincipalStrain [4]
__global__ __launch_bounds__(64) void k_stress_strain(ElemArrays ea, ElemParams ep, const double* __restrict__ U, int64_t ncell,
                                                      const int32_t* __restrict__ cells, double* __restrict__ out) {
  const int64_t ci = blockIdx.x;
  stress_strain_cell(ea, ep, U, cells[ci], out + ci * 80);
}

// One lane per boundary cell: fmask bit f set = the facet opposite local vertex f is an exterior facet.
// out[c][4][3]: DG1 coefficients of the projected tangential traction (0 on vertices that touch no exterior facet).
__global__ __launch_bounds__(64) void k_wss(ElemArrays ea, const double* __restrict__ U, int64_t ncell,
                                            const int32_t* __restrict__ cells, const int32_t* __restrict__ fmask, double mu,
                                            double* __restrict__ out) {
  const int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (ci >= ncell) return;
  double b[4][3];
  wss_dg1_cell(ea, U, cells[ci], fmask[ci], mu, b);
  for (int a = 0; a < 4; ++a)
    for (int i = 0; i < 3; ++i) out[(ci * 4 + a) * 3 + i] = b[a][i];
}

}  // namespace

hipError_t upload_post_tables(const double* qw, const double* dN, const double* L) {
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(p_qw), qw, sizeof(double) * NQ);
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(p_dN), dN, sizeof(double) * NQ * 30);
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(p_L), L, sizeof(double) * NQ * 4);
  if (e == hipSuccess) e = upload_stress_tables(qw, dN, L);          // the copies of fsi_stress.hip (fsi_stress.hpp)
  p_tables_ready = e == hipSuccess;
  return e;
}
void launch_stress_strain(hipStream_t st, int64_t ncell, const ElemArrays& ea, const ElemParams& ep, const double* U,
                          const int32_t* cells, double* out) {
  if (ncell > 0) hipLaunchKernelGGL(k_stress_strain, dim3((unsigned)ncell), dim3(64), 0, st, ea, ep, U, ncell, cells, out);
}
void launch_wss(hipStream_t st, int64_t ncell, const ElemArrays& ea, const double* U, const int32_t* cells, const int32_t* fmask,
                double mu, double* out) {
  if (ncell > 0)
    hipLaunchKernelGGL(k_wss, dim3((unsigned)((ncell + 63) / 64)), dim3(64), 0, st, ea, U, ncell, cells, fmask, mu, out);
}

}  // namespace fsi
