// Hemodynamic indices accumulated on the device during a run (second half).
//
// Replaces the time loop and the closing arithmetic of compute_hemodyanamics
// [REF src/vasp/postprocessing/postprocessing_fenics/compute_hemodynamics.py:160-372]: per saved frame the wall shear
// stress tau (the DG1-projected tangential traction of Stress, the arithmetic of k_wss through wss_dg1_cell) and the sums
// behind TAWSS, OSI, RRT, ECAP and TWSSG; at the end the indices per DG1 dof of the boundary mesh.
//
//   k_hemo_sample : one lane per boundary cell.  The cell's DG1 traction b[4][3] is evaluated once; then, at the three
//                   vertices k of every listed exterior facet fi of the cell (dof d = 3 fi + k):
//                     sum_tau[d]   += tau                      (WSS_mean.vector().axpy)
//                     sum_mag[d]   += |tau|                    (np.linalg.norm of the nodal vector, :268-280)
//                     sum_twssg[d] += P1 projection on the facet of |(tau - tau_prev) / dt| (project_dg, :282-287)
//                     tau_prev[d]   = tau
//                   The projection integrates the norm of the linear DG1 difference at the 12 points of the degree-6
//                   triangle rule (oracle.fsi_oracle.triangle12, uploaded by hemo_upload_tables) and applies the inverse
//                   of the P1 mass matrix of a triangle, M = A/12 (I + 1 1^T), M^-1 = (3/A)(4 I - 1 1^T): with the
//                   physical weights 2 A w_q the area cancels, proj_a = 6 sum_b (4 delta_ab - 1) sum_q w_q L_qb |D_q|.
//                   Quirk kept from the reference: tau_prev starts at zero (:244), so the first sample adds |tau_1| / dt
//                   to TWSSG (:309-316).
//   k_spec_wss_sample : one lane per boundary cell touched by the sampled dofs of a spectrogram session (--spectrogram wss):
//                   the same b, written to the session's rows of hist[frame] - a component or the magnitude of a dof.
//   k_hemo_finish : one lane per dof, plain IEEE arithmetic as the reference's numpy (inf / NaN where a denominator
//                   vanishes, no clamping): TAWSS = sum_mag / n, m = |sum_tau / n|, RRT = 1 / m, OSI = (1 - m / TAWSS) / 2,
//                   ECAP = OSI / TAWSS, TWSSG = sum_twssg / n.
//
// Every facet belongs to exactly one boundary cell, hence to one lane: no atomics, and the indices of a run are bitwise
// reproducible run to run.  Geometry is the undeformed mesh (ea.geom), as the reference's post-processing reads
// Mesh/mesh.h5.  Accumulators per dof: sum_tau 3 + tau_prev 3 + sum_mag 1 + sum_twssg 1 doubles, all read and written
// once per sample (8 * 8 * 2 = 128 B per dof, 384 B per facet), plus the traction's gather of 30 velocity values and 10
// geometry doubles per boundary cell.
#include "fsi_kernels.hpp"
#include "fsi_wss.hpp"

namespace fsi {

namespace {

constexpr int NT = 12;          // points of the degree-6 triangle rule
__constant__ double h_tw[NT];   // weights (sum 1/2)
__constant__ double h_tl[NT][3];  // barycentric coordinates (1 - x - y, x, y)

__constant__ int c_fverts[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};

__global__ __launch_bounds__(64) void k_hemo_sample(ElemArrays ea, const double* __restrict__ U, int64_t ncell,
                                                    const int32_t* __restrict__ cells, const int32_t* __restrict__ fmask,
                                                    const int32_t* __restrict__ fidx, double mu, double dt, HemoAcc acc,
                                                    double* __restrict__ wss_out) {
  const int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (ci >= ncell) return;
  const int mask = fmask[ci];
  double b[4][3];
  wss_dg1_cell(ea, U, cells[ci], mask, mu, b);
  for (int f = 0; f < 4; ++f) {
    if (!(mask & (1 << f))) continue;
    const int64_t d0 = 3 * (int64_t)fidx[ci * 4 + f];          // first dof of the facet (user order)
    double D[3][3];                                            // (tau - tau_prev) / dt at the facet's vertices
    for (int k = 0; k < 3; ++k) {
      const int a = c_fverts[f][k];
      const int64_t d = d0 + k;
      double s2 = 0.0;
      for (int i = 0; i < 3; ++i) {
        const double t = b[a][i];
        D[k][i] = (t - acc.tau_prev[3 * d + i]) / dt;
        acc.sum_tau[3 * d + i] += t;
        acc.tau_prev[3 * d + i] = t;
        if (wss_out) wss_out[3 * d + i] = t;
        s2 += t * t;
      }
      acc.sum_mag[d] += sqrt(s2);
    }
    double r[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < NT; ++q) {
      double g2 = 0.0;
      for (int i = 0; i < 3; ++i) {
        const double x = h_tl[q][0] * D[0][i] + h_tl[q][1] * D[1][i] + h_tl[q][2] * D[2][i];
        g2 += x * x;
      }
      const double wg = h_tw[q] * sqrt(g2);
      for (int k = 0; k < 3; ++k) r[k] += wg * h_tl[q][k];
    }
    const double rs = r[0] + r[1] + r[2];
    for (int k = 0; k < 3; ++k) acc.sum_twssg[d0 + k] += 6.0 * (4.0 * r[k] - rs);
  }
}

// The rows of a spectrogram session of the wall shear stress (fsi_spec_begin_wss): one lane per boundary cell that a sampled
// dof touches.  fmask is the cell's full exterior-facet mask, so b is what k_wss and k_hemo_sample form on the cell, whichever
// of its dofs are sampled; the lane then writes its own rows - a dof drawn twice is two entries of its list.
__global__ __launch_bounds__(64) void k_spec_wss_sample(ElemArrays ea, const double* __restrict__ U, int64_t ncell,
                                                        const int32_t* __restrict__ cells, const int32_t* __restrict__ fmask,
                                                        const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent, double mu,
                                                        double* __restrict__ dst) {
  const int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (ci >= ncell) return;
  double b[4][3];
  wss_dg1_cell(ea, U, cells[ci], fmask[ci], mu, b);
  for (int32_t e = ptr[ci]; e < ptr[ci + 1]; ++e) {
    const int32_t row = ent[2 * e], code = ent[2 * e + 1], va = code >> 2, comp = code & 3;
    double t[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 4; ++a)                                // selects, not indexing: b stays in registers
      for (int i = 0; i < 3; ++i)
        if (a == va) t[i] = b[a][i];
    double val;
    if (comp == 3) {
#pragma clang fp contract(off)                                 // the arithmetic of k_spec_magnitude (fsi_spec.hip), bit for bit
      val = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    } else {
      val = comp == 0 ? t[0] : comp == 1 ? t[1] : t[2];
    }
    dst[row] = val;
  }
}

// out[5][ndof]: TAWSS, OSI, RRT, ECAP, TWSSG
__global__ __launch_bounds__(256) void k_hemo_finish(int64_t ndof, double n, HemoAcc acc, double* __restrict__ out) {
  const int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (d >= ndof) return;
  const double tawss = acc.sum_mag[d] / n;
  const double mx = acc.sum_tau[3 * d] / n, my = acc.sum_tau[3 * d + 1] / n, mz = acc.sum_tau[3 * d + 2] / n;
  const double m = sqrt(mx * mx + my * my + mz * mz);
  const double osi = 0.5 * (1.0 - m / tawss);
  out[d] = tawss;
  out[ndof + d] = osi;
  out[2 * ndof + d] = 1.0 / m;
  out[3 * ndof + d] = osi / tawss;
  out[4 * ndof + d] = acc.sum_twssg[d] / n;
}

}  // namespace

hipError_t hemo_upload_tables(const double* w, const double* lam) {     // on the current device, at every fsi_hemo_begin
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(h_tw), w, sizeof(double) * NT);
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(h_tl), lam, sizeof(double) * NT * 3);
}
void launch_hemo_sample(hipStream_t st, int64_t ncell, const ElemArrays& ea, const double* U, const int32_t* cells,
                        const int32_t* fmask, const int32_t* fidx, double mu, double dt, const HemoAcc& acc, double* wss_out) {
  if (ncell > 0)
    hipLaunchKernelGGL(k_hemo_sample, dim3((unsigned)((ncell + 63) / 64)), dim3(64), 0, st, ea, U, ncell, cells, fmask, fidx,
                       mu, dt, acc, wss_out);
}
void launch_spec_wss_sample(hipStream_t st, int64_t ncell, const ElemArrays& ea, const double* U, const int32_t* cells,
                            const int32_t* fmask, const int32_t* ptr, const int32_t* ent, double mu, double* dst) {
  if (ncell > 0)
    hipLaunchKernelGGL(k_spec_wss_sample, dim3((unsigned)((ncell + 63) / 64)), dim3(64), 0, st, ea, U, ncell, cells, fmask, ptr, ent,
                       mu, dst);
}
void launch_hemo_finish(hipStream_t st, int64_t ndof, double samples, const HemoAcc& acc, double* out) {
  if (ndof > 0)
    hipLaunchKernelGGL(k_hemo_finish, dim3((unsigned)((ndof + 255) / 256)), dim3(256), 0, st, ndof, samples, acc, out);
}

}  // namespace fsi
