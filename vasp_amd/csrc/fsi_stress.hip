// Solid stress and strain sampled on the device during a run.
//
// Replaces the frame loop and the closing averages of compute_stress_strain
// [REF src/vasp/postprocessing/postprocessing_fenics/compute_stress_strain.py:188-290]: per saved frame the DG1 Cauchy stress,
// Green-Lagrange strain and their largest principal values on the session's solid cells (the arithmetic of k_stress_strain
// through stress_strain_cell), and the running sums behind MaxPrincipalStress_avg / MaxPrincipalStrain_avg.
//
//   k_stress_sample  : one 64-lane workgroup per listed solid cell, as k_stress_strain.  The frame goes to frame[ci][80] in
//                      HBM (the fsi_stress_strain layout); lanes 0..7 add the cell's eight principal values to
//                      sums[ci][8] (MPStress_avg.vector().axpy(1.0, ...), :246-248).
//   k_stress_average : one lane per averaged value: out[t][ci][a] = sums[ci][4 t + a] / n (the `/ counter` of :255-257).
//
// And the two kernels of a band-pass session on a tensor (fsi_band_begin_cells, quantity FSI_BAND_STRAIN / FSI_BAND_STRESS),
// which replace the component matrices create_transformed_matrix builds from the StressStrain files
// [REF src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:250-259,349-354] and the eigenvalue loop of
// create_hi_pass_viz [REF src/vasp/postprocessing/postprocessing_h5py/create_hi_pass_viz.py:295-314]:
//
//   k_tensor_sample    : one 64-lane workgroup per listed solid cell; the tensors of stress_strain_cell go to LDS, and lanes
//                        0..23 write the 24 rows of the cell, row (4 ci + a) 6 + comp = entry 0, 1, 4, 5, 8, 6 (11, 12, 22,
//                        23, 33, 31) of dof a of the asked tensor: 192 contiguous bytes per cell.  Here, because the Keast
//                        tables of stress_strain_cell are this unit's copies.
//   k_tensor_principal : one lane per DG1 dof: from its six amplitudes T = [[11,12,31],[12,22,23],[31,23,33]]; exactly 0 where
//                        every |T_ij| < 1e-8, else max_eig_sym3(T) (get_eig).
//
// Every sum slot belongs to one lane of one workgroup and the samples are stream-ordered: no atomics, and the averages are
// the sequential sums of the sampled values divided by n, bit for bit, run to run.  HBM traffic per cell and sample: the
// gather of k_stress_strain (30 displacement values, 10 geometry doubles, the cell's dof row and region) in, 80 doubles
// of frame out, 8 sums read and written.
#include "fsi_kernels.hpp"
#include "fsi_stress.hpp"

namespace fsi {

namespace {

__global__ __launch_bounds__(64) void k_stress_sample(ElemArrays ea, ElemParams ep, const double* __restrict__ U,
                                                      const int32_t* __restrict__ cells, double* __restrict__ frame,
                                                      double* __restrict__ sums) {
  const int64_t ci = blockIdx.x;
  const double pv = stress_strain_cell(ea, ep, U, cells[ci], frame + ci * 80);
  if (threadIdx.x < 8) {
#pragma clang fp contract(off)   // add the value the frame holds: contracted, the sum would take pv's last product unrounded
    sums[ci * 8 + threadIdx.x] += pv;
  }
}

// out[2][n][4]: MaxPrincipalStress_avg, MaxPrincipalStrain_avg
__global__ __launch_bounds__(256) void k_stress_average(int64_t n, double samples, const double* __restrict__ sums,
                                                        double* __restrict__ out) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= 8 * n) return;
  const int64_t t = k / (4 * n), r = k % (4 * n), ci = r / 4, a = r % 4;
  out[k] = sums[ci * 8 + 4 * t + a] / samples;
}

__global__ __launch_bounds__(64) void k_tensor_sample(ElemArrays ea, ElemParams ep, const double* __restrict__ U,
                                                      const int32_t* __restrict__ cells, int strain, double* __restrict__ dst) {
  __shared__ double oc[72];
  const int64_t ci = blockIdx.x;
  stress_strain_cell<false>(ea, ep, U, cells[ci], oc);
  __syncthreads();
  const int r = threadIdx.x;
  if (r < 24) {
    const int entry[6] = {0, 1, 4, 5, 8, 6};             // the tensors are not bitwise symmetric: 31 is entry 6, 12 entry 1
    dst[ci * 24 + r] = oc[(strain ? 36 : 0) + (r / 6) * 9 + entry[r % 6]];
  }
}

__global__ __launch_bounds__(256) void k_tensor_principal(int64_t nnode, const double* __restrict__ amp, double* __restrict__ mag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnode) return;
  const double* a = amp + 6 * i;                         // 11, 12, 22, 23, 33, 31
  const double T[3][3] = {{a[0], a[1], a[5]}, {a[1], a[2], a[3]}, {a[5], a[3], a[4]}};
  bool zero = true;
  for (int k = 0; k < 6; ++k) zero = zero && fabs(a[k]) < 1e-8;
  mag[i] = zero ? 0.0 : max_eig_sym3(T);
}

}  // namespace

hipError_t upload_stress_tables(const double* qw, const double* dN, const double* L) {   // this unit's copies, at create
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(p_qw), qw, sizeof(double) * NQ);
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(p_dN), dN, sizeof(double) * NQ * 30);
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(p_L), L, sizeof(double) * NQ * 4);
}
void launch_stress_sample(hipStream_t st, int64_t ncell, const ElemArrays& ea, const ElemParams& ep, const double* U,
                          const int32_t* cells, double* frame, double* sums) {
  if (ncell > 0) hipLaunchKernelGGL(k_stress_sample, dim3((unsigned)ncell), dim3(64), 0, st, ea, ep, U, cells, frame, sums);
}
void launch_stress_average(hipStream_t st, int64_t ncell, double samples, const double* sums, double* out) {
  if (ncell > 0)
    hipLaunchKernelGGL(k_stress_average, dim3((unsigned)((8 * ncell + 255) / 256)), dim3(256), 0, st, ncell, samples, sums, out);
}

void launch_tensor_sample(hipStream_t st, int64_t ncell, const ElemArrays& ea, const ElemParams& ep, const double* U,
                          const int32_t* cells, bool strain, double* dst) {
  if (ncell > 0) hipLaunchKernelGGL(k_tensor_sample, dim3((unsigned)ncell), dim3(64), 0, st, ea, ep, U, cells, strain ? 1 : 0, dst);
}
void launch_tensor_principal(hipStream_t st, int64_t nnode, const double* amp, double* mag) {
  if (nnode > 0) hipLaunchKernelGGL(k_tensor_principal, dim3((unsigned)((nnode + 255) / 256)), dim3(256), 0, st, nnode, amp, mag);
}

}  // namespace fsi
