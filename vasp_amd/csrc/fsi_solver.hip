// Sparse and vector kernels of the linear solve (gfx950): CSR expansion, BLAS-1, row equilibration and boundary rows, the
// deterministic reductions, ILU(0) factorisation and triangular solves, and the streams that calibrate the byte counters.
// (The products with the monolithic matrix and the generic CSR product are in fsi_product.hip.)
//
// Replaces what PETSc/MUMPS do behind `up_sol.set_operator(A)` / `up_sol.solve(dvp_res.vector(), b)` in turtleFSI's
// newtonsolver.  All of these kernels are HBM-bound; algorithmic bytes per call:
//   SpTRSV   (nnz/2)*(8+4) + n*24           per triangle
//   dot      n*16
// The factorisation and the triangular solves run colour by colour on a multicolour ordering of the mesh nodes
// (one launch per colour, one wave per node, no spinning): see k_ilu0_level / k_sptrsv_level.
#include <algorithm>

#include "fsi_kernels.hpp"

namespace fsi {

static constexpr int MAXROW = 1024;

__device__ inline double ld_agent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_agent(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline unsigned long long ld_agent_bits(const double* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline double wave_sum(double v) { return wave_sum_dpp(v); }      // DPP row sums + four lane reads, wave-uniform
__device__ inline double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// ---------------------------------------------------------------------------------------------------------
// CSR structure from the node graph.  Row of any dof of node (rank r): for every neighbour rank s (ascending) the
// six columns 6s..6s+5 (d_x d_y d_z v_x v_y v_z), then the pressure columns 6*N2 + u of its vertex neighbours.
// ---------------------------------------------------------------------------------------------------------
__global__ void k_expand_cols(int64_t N2, int64_t V, const int64_t* __restrict__ nadj_ptr,
                              const int32_t* __restrict__ nadj, const int64_t* __restrict__ padj_ptr,
                              const int32_t* __restrict__ padj, const int32_t* __restrict__ vrank,
                              const int64_t* __restrict__ rowptr, int32_t* __restrict__ cols,
                              int64_t* __restrict__ diagpos) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t n = 6 * N2 + V;
  if (row >= n) return;
  const bool isp = row >= 6 * N2;
  const int32_t r = isp ? vrank[row - 6 * N2] : (int32_t)(row / 6);
  const int t = isp ? 0 : (int)(row % 6);
  int64_t pos = rowptr[row];
  for (int64_t k = nadj_ptr[r]; k < nadj_ptr[r + 1]; ++k) {
    const int32_t s = nadj[k];
    if (!isp && s == r) diagpos[row] = pos + t;
    for (int e = 0; e < 6; ++e) cols[pos++] = 6 * s + e;
  }
  for (int64_t k = padj_ptr[r]; k < padj_ptr[r + 1]; ++k) {
    const int32_t u = padj[k];
    if (isp && u == row - 6 * N2) diagpos[row] = pos;
    cols[pos++] = (int32_t)(6 * N2 + u);
  }
}

// ---------------------------------------------------------------------------------------------------------
// vector kernels
// ---------------------------------------------------------------------------------------------------------
#define GRID_STRIDE(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ void k_fill(double* x, int64_t n, double v) { GRID_STRIDE(i, n) x[i] = v; }
__global__ void k_fill_bits(double* x, int64_t n, unsigned long long v) {
  GRID_STRIDE(i, n) reinterpret_cast<unsigned long long*>(x)[i] = v;
}
__global__ void k_copy(double* d, const double* s, int64_t n) { GRID_STRIDE(i, n) d[i] = s[i]; }
__global__ void k_axpy(double* y, double a, const double* x, int64_t n) { GRID_STRIDE(i, n) y[i] += a * x[i]; }
__global__ void k_axpby(double* z, double a, const double* x, double b, const double* y, int64_t n) {
  GRID_STRIDE(i, n) z[i] = a * x[i] + b * y[i];
}
__global__ void k_scale(double* y, double a, int64_t n) { GRID_STRIDE(i, n) y[i] *= a; }
__global__ void k_mul(double* z, const double* x, const double* y, int64_t n) { GRID_STRIDE(i, n) z[i] = x[i] * y[i]; }
__global__ void k_div(double* z, const double* x, const double* y, int64_t n) { GRID_STRIDE(i, n) z[i] = x[i] / y[i]; }
__global__ void k_gather(double* d, const double* s, const int32_t* idx, int64_t n) { GRID_STRIDE(i, n) d[i] = s[idx[i]]; }
__global__ void k_scatter(double* d, const double* s, const int32_t* idx, int64_t n) { GRID_STRIDE(i, n) d[idx[i]] = s[i]; }
// the targets are distinct (merged on the host): plain adds
__global__ void k_add_indexed(double* y, const int32_t* idx, const double* coef, double a, int64_t n) {
  GRID_STRIDE(i, n) y[idx[i]] += a * coef[i];
}
__global__ void k_negate(double* b, const double* F, int64_t n) { GRID_STRIDE(i, n) b[i] = -F[i]; }
__global__ void k_bc_rhs(double* b, const double* U, const int32_t* bc, const double* g, int64_t n) {
  GRID_STRIDE(i, n) b[bc[i]] = g[i] - U[bc[i]];
}
__global__ void k_bc_set(double* U, const int32_t* bc, const double* g, int64_t n) { GRID_STRIDE(i, n) U[bc[i]] = g[i]; }
__global__ void k_mark(int32_t* mask, const int32_t* idx, int64_t n) { GRID_STRIDE(i, n) mask[idx[i]] = 1; }
__global__ void k_izero(int32_t* x, int64_t n) { GRID_STRIDE(i, n) x[i] = 0; }
// one thread per distinct row: its entries (sorted by column on the host) are added in that order
__global__ void k_robin_residual(int64_t nrows, const int32_t* urow, const int32_t* ptr, const int32_t* col, const double* val,
                                 double th0, double th1, const double* U, const double* U1, double* F) {
  GRID_STRIDE(k, nrows) {
    double s = 0.0;
    for (int32_t i = ptr[k]; i < ptr[k + 1]; ++i) s += val[i] * (th0 * U[col[i]] + th1 * U1[col[i]]);
    F[urow[k]] += s;
  }
}
__global__ void k_add_at(double* vals, const int64_t* pos, const double* v, double a, int64_t n) {     // distinct positions
  GRID_STRIDE(i, n) vals[pos[i]] += a * v[i];
}

static inline unsigned grid_for(int64_t n, int bs = 256) {
  int64_t g = (n + bs - 1) / bs;
  if (g < 1) g = 1;
  if (g > 4096) g = 4096;
  return (unsigned)g;
}
#define LAUNCH1D(kern, st, n, ...) hipLaunchKernelGGL(kern, dim3(grid_for(n)), dim3(256), 0, st, __VA_ARGS__)

void launch_expand_cols(hipStream_t st, int64_t N2, int64_t V, const int64_t* nadj_ptr, const int32_t* nadj,
                        const int64_t* padj_ptr, const int32_t* padj, const int32_t* vrank, const int64_t* rowptr,
                        int32_t* cols, int64_t* diagpos) {
  const int64_t n = 6 * N2 + V;
  if (n > 0) hipLaunchKernelGGL(k_expand_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, N2, V, nadj_ptr, nadj,
                     padj_ptr, padj, vrank, rowptr, cols, diagpos);
}
void launch_fill(hipStream_t st, double* x, int64_t n, double v) { LAUNCH1D(k_fill, st, n, x, n, v); }
void launch_copy(hipStream_t st, double* d, const double* s, int64_t n) { LAUNCH1D(k_copy, st, n, d, s, n); }
void launch_axpy(hipStream_t st, double* y, double a, const double* x, int64_t n) { LAUNCH1D(k_axpy, st, n, y, a, x, n); }
void launch_axpby(hipStream_t st, double* z, double a, const double* x, double b, const double* y, int64_t n) {
  LAUNCH1D(k_axpby, st, n, z, a, x, b, y, n);
}
void launch_scale(hipStream_t st, double* y, double a, int64_t n) { LAUNCH1D(k_scale, st, n, y, a, n); }
void launch_mul(hipStream_t st, double* z, const double* x, const double* y, int64_t n) { LAUNCH1D(k_mul, st, n, z, x, y, n); }
void launch_div(hipStream_t st, double* z, const double* x, const double* y, int64_t n) { LAUNCH1D(k_div, st, n, z, x, y, n); }
void launch_gather(hipStream_t st, double* d, const double* s, const int32_t* idx, int64_t n) { LAUNCH1D(k_gather, st, n, d, s, idx, n); }
void launch_scatter(hipStream_t st, double* d, const double* s, const int32_t* idx, int64_t n) { LAUNCH1D(k_scatter, st, n, d, s, idx, n); }
void launch_add_indexed(hipStream_t st, double* y, const int32_t* idx, const double* coef, double a, int64_t n) {
  if (n > 0) LAUNCH1D(k_add_indexed, st, n, y, idx, coef, a, n);
}
void launch_negate(hipStream_t st, double* b, const double* F, int64_t n) { LAUNCH1D(k_negate, st, n, b, F, n); }
void launch_bc_rhs(hipStream_t st, double* b, const double* U, const int32_t* bc, const double* g, int64_t n) {
  if (n > 0) LAUNCH1D(k_bc_rhs, st, n, b, U, bc, g, n);
}
void launch_bc_set(hipStream_t st, double* U, const int32_t* bc, const double* g, int64_t n) {
  if (n > 0) LAUNCH1D(k_bc_set, st, n, U, bc, g, n);
}
void launch_robin_residual(hipStream_t st, int64_t nrows, const int32_t* urow, const int32_t* ptr, const int32_t* col,
                           const double* val, double th0, double th1, const double* U, const double* U1, double* F) {
  if (nrows > 0) LAUNCH1D(k_robin_residual, st, nrows, nrows, urow, ptr, col, val, th0, th1, U, U1, F);
}
void launch_add_at(hipStream_t st, double* vals, const int64_t* pos, const double* v, double a, int64_t n) {
  if (n > 0) LAUNCH1D(k_add_at, st, n, vals, pos, v, a, n);
}

// ---------------------------------------------------------------------------------------------------------
// A = Jn + Apre ; ident_zeros ; Dirichlet rows -> identity ; row equilibration.   One wave per row.
// (DOLFIN: A.axpy(1.0, A_pre, True); A.ident_zeros(); [bc.apply(A) for bc in bcs])
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_matrix_finish(int64_t n, const int64_t* __restrict__ rowptr,
                                                       const int64_t* __restrict__ diagpos, double* __restrict__ A,
                                                       const double* __restrict__ Apre,
                                                       const int32_t* __restrict__ bcmask, double* __restrict__ rowscale) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < n; row += nwaves) {
    const int64_t s = rowptr[row], e = rowptr[row + 1], dp = diagpos[row];
    double mx = 0.0;
    for (int64_t t = s + lane; t < e; t += 64) {
      const double v = A[t] + Apre[t];
      A[t] = v;
      mx = fmax(mx, fabs(v));
    }
    mx = wave_max(mx);
    const bool ident = (mx < 3.0e-16) || bcmask[row];     // DOLFIN_EPS
    if (ident) {
      for (int64_t t = s + lane; t < e; t += 64) A[t] = (t == dp) ? 1.0 : 0.0;
      if (lane == 0) rowscale[row] = 1.0;
    } else {
      const double sc = 1.0 / mx;
      for (int64_t t = s + lane; t < e; t += 64) A[t] *= sc;
      if (lane == 0) rowscale[row] = sc;
    }
  }
}
void launch_matrix_finish(hipStream_t st, int64_t n, const int64_t* rowptr, const int64_t* diagpos, double* A,
                          const double* Apre, const int32_t* bc, int64_t nbc, double* rowscale, int32_t* bcmask) {
  LAUNCH1D(k_izero, st, n, bcmask, n);
  if (nbc > 0) LAUNCH1D(k_mark, st, nbc, bcmask, bc, nbc);
  hipLaunchKernelGGL(k_matrix_finish, dim3(grid_for(n * 64)), dim3(256), 0, st, n, rowptr, diagpos, A, Apre, bcmask, rowscale);
}

// ---------------------------------------------------------------------------------------------------------
// deterministic reductions
// ---------------------------------------------------------------------------------------------------------
__device__ inline double block_sum(double v) {
  __shared__ double sh[4];
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void k_dot_partial(const double* __restrict__ x, const double* __restrict__ y,
                                                     int64_t n, double* __restrict__ part) {
  double s = 0.0;
  GRID_STRIDE(i, n) s += x[i] * y[i];
  s = block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_sum_final(const double* __restrict__ part, int np, int stride,
                                                   double* __restrict__ out) {
  // block b sums part[b*stride .. b*stride+np)
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) s += part[(int64_t)blockIdx.x * stride + i];
  s = block_sum(s);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
// sum_i x[first + i * stride] * w(i) with an index-dependent weight in [1, 2) (a multiplicative hash of i): unlike a sum
// of squares this sees sign changes, permuted entries and, through the weights, which entry a change sits in
__global__ __launch_bounds__(256) void k_hashed_sum_partial(const double* __restrict__ x, int64_t first, int64_t stride, int64_t n,
                                                            double* __restrict__ part) {
  double s = 0.0;
  GRID_STRIDE(i, n) {
    const uint32_t h = (uint32_t)((uint64_t)i * 0x9E3779B97F4A7C15ull >> 40);      // 24 bits
    s += x[first + i * stride] * (1.0 + (double)h * (1.0 / 16777216.0));
  }
  s = block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
void launch_hashed_sum(hipStream_t st, const double* x, int64_t first, int64_t stride, int64_t n, double* scratch, double* out) {
  int np = (int)grid_for(n);
  if (np > 1024) np = 1024;
  hipLaunchKernelGGL(k_hashed_sum_partial, dim3(np), dim3(256), 0, st, x, first, stride, n, scratch);
  hipLaunchKernelGGL(k_sum_final, dim3(1), dim3(256), 0, st, scratch, np, np, out);
}
void launch_dot(hipStream_t st, const double* x, const double* y, int64_t n, double* scratch, double* out) {
  int np = (int)grid_for(n);
  if (np > 1024) np = 1024;
  hipLaunchKernelGGL(k_dot_partial, dim3(np), dim3(256), 0, st, x, y, n, scratch);
  hipLaunchKernelGGL(k_sum_final, dim3(1), dim3(256), 0, st, scratch, np, np, out);
}
// ---------------------------------------------------------------------------------------------------------
// ILU(0) and triangular solves on a multicolour ordering.
//
// Rows are numbered colour by colour (fsi_create): nodes of one colour share no element, so their rows do not
// reference each other and a whole colour is processed by one launch, one wave per node.  The (up to) six rows of a
// node are mutually coupled and are processed in order by that wave; what it hands from one of its rows to the next
// goes through agent-scope stores/loads (write-through, L1-bypassing), drained with s_waitcnt before the next row.
// Launch boundaries order the colours, so there is no spinning anywhere.
// counters[1]: error flags (1 = row too long, 2 = zero / non-finite pivot).
// Every row must have a diagonal entry (diagpos[row] >= rowptr[row]): the kernel indexes its LDS tile with
// diagpos[row] - rowptr[row].  The library's matrix has one in every row before any factorisation runs, by construction
// in fsi_create: number_nodes (fsi_setup.hip) puts the pair (a, a) of every node of every cell into the node graph and
// refuses a node that belongs to no cell, so every node is its own neighbour and k_expand_cols finds the diagonal of its
// six rows; a vertex is then its own pressure neighbour too (build_node_graph keeps the neighbours below V), and
// build_pressure_blocks refuses a context ("vertex missing from its own neighbour list") where it is not.  The -1 that
// k_expand_cols leaves in a row without a diagonal therefore never reaches a context that refresh_preconditioner sees;
// k_matrix_finish / ident_zeros only decide the VALUE of that entry (1 in an all-zero or Dirichlet row).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ilu0_level(int64_t first_row, int64_t ngroups, int group_rows,
                                                   const int64_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ cols,
                                                   const int64_t* __restrict__ diagpos, double* __restrict__ LU,
                                                   int32_t* __restrict__ counters) {
  __shared__ int32_t s_cols[MAXROW];
  __shared__ double s_vals[MAXROW];
  volatile double* sv = s_vals;
  const int lane = threadIdx.x;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    for (int rr = 0; rr < group_rows; ++rr) {
      const int64_t row = first_row + g * group_rows + rr;
      const int64_t s = rowptr[row];
      const int len = (int)(rowptr[row + 1] - s);
      const int nlow = (int)(diagpos[row] - s);
      if (len > MAXROW) {
        if (lane == 0) atomicOr(&counters[1], 1);
        continue;
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < len; t += 64) { s_cols[t] = cols[s + t]; s_vals[t] = LU[s + t]; }
      __builtin_amdgcn_wave_barrier();
      for (int t = 0; t < nlow; ++t) {
        const int32_t k = s_cols[t];
        const int64_t dk = diagpos[k];
        const double ukk = ld_agent(&LU[dk]);
        const double l = sv[t] / ukk;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) sv[t] = l;
        if (l != 0.0) {
          const int64_t ke = rowptr[k + 1];
          for (int64_t q = dk + 1 + lane; q < ke; q += 64) {
            const int32_t j = cols[q];
            const double u = ld_agent(&LU[q]);
            int lo = t + 1, hi = len - 1;            // binary search for column j in this row
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (s_cols[mid] < j) lo = mid + 1; else hi = mid;
            }
            if (lo < len && s_cols[lo] == j) sv[lo] -= l * u;
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      const double piv = sv[nlow];
      if (!(fabs(piv) > 0.0) || !isfinite(piv)) {
        if (lane == 0) { atomicOr(&counters[1], 2); sv[nlow] = 1.0; }
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < len; t += 64) st_agent(&LU[s + t], sv[t]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
}

// L (unit diagonal) y = rhs on one colour, or U x = y on one colour (groups and rows in reverse).
template <bool UPPER>
__global__ __launch_bounds__(256) void k_sptrsv_level(int64_t first_row, int64_t ngroups, int group_rows,
                                                      const int64_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ cols,
                                                      const int64_t* __restrict__ diagpos,
                                                      const double* __restrict__ LU, const double* __restrict__ rhs,
                                                      double* __restrict__ x) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    const int64_t g0 = first_row + g * group_rows;
    for (int rr = 0; rr < group_rows; ++rr) {
      const int64_t row = UPPER ? g0 + group_rows - 1 - rr : g0 + rr;
      const int64_t dp = diagpos[row];
      const int64_t s = UPPER ? dp + 1 : rowptr[row];
      const int64_t e = UPPER ? rowptr[row + 1] : dp;
      double sum = 0.0;
      for (int64_t t = s + lane; t < e; t += 64) {
        const int32_t c = cols[t];
        // values of this node's own rows were stored a moment ago by this wave: read them past L1
        const double xv = (c >= g0 && c < g0 + group_rows) ? ld_agent(&x[c]) : x[c];
        sum += LU[t] * xv;
      }
      sum = wave_sum(sum);
      if (lane == 0) {
        double v = rhs[row] - sum;
        if (UPPER) v /= LU[dp];
        st_agent(&x[row], v);
      }
      if (group_rows > 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
}

void launch_ilu0_levels(hipStream_t st, const std::vector<Level>& levels, const int64_t* rowptr, const int32_t* cols,
                        const int64_t* diagpos, double* LU, int32_t* counters) {
  LAUNCH1D(k_izero, st, 4, counters, (int64_t)4);
  for (const Level& L : levels) {
    if (L.ngroups == 0) continue;
    const unsigned blocks = (unsigned)std::min<int64_t>(L.ngroups, 16384);
    hipLaunchKernelGGL(k_ilu0_level, dim3(blocks), dim3(64), 0, st, L.first_row, L.ngroups, L.group_rows, rowptr, cols,
                       diagpos, LU, counters);
  }
}
void launch_sptrsv_levels(hipStream_t st, const std::vector<Level>& levels, const int64_t* rowptr, const int32_t* cols,
                          const int64_t* diagpos, const double* LU, const double* rhs, double* tmp, double* x) {
  for (size_t i = 0; i < levels.size(); ++i) {
    const Level& L = levels[i];
    if (L.ngroups == 0) continue;
    const unsigned blocks = (unsigned)std::min<int64_t>((L.ngroups + 3) / 4, 8192);
    hipLaunchKernelGGL(k_sptrsv_level<false>, dim3(blocks), dim3(256), 0, st, L.first_row, L.ngroups, L.group_rows,
                       rowptr, cols, diagpos, LU, rhs, tmp);
  }
  for (size_t i = levels.size(); i-- > 0;) {
    const Level& L = levels[i];
    if (L.ngroups == 0) continue;
    const unsigned blocks = (unsigned)std::min<int64_t>((L.ngroups + 3) / 4, 8192);
    hipLaunchKernelGGL(k_sptrsv_level<true>, dim3(blocks), dim3(256), 0, st, L.first_row, L.ngroups, L.group_rows,
                       rowptr, cols, diagpos, LU, tmp, x);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Known-byte streams for calibrating the rocprofv3 FETCH_SIZE / WRITE_SIZE counters at the access widths the solver
// kernels use (MI355X_MICROARCH.md: exact for some widths, half for 16-byte-per-lane reads, uncalibrated otherwise).
// Each kernel reads (writes) exactly `bytes` once, W bytes per lane and instruction, grid-stride.
// ---------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_cal_read(const T* __restrict__ src, int64_t count, double* __restrict__ out) {
  double acc = 0.0;
  GRID_STRIDE(i, count) {
    const T v = src[i];
    acc += (double)reinterpret_cast<const float*>(&v)[0];
  }
  if (acc == 12345.678) out[0] = acc;         // keeps the loads alive without a store per thread
}
template <class T>
__global__ __launch_bounds__(256) void k_cal_write(T* __restrict__ dst, int64_t count) {
  T v;
  for (size_t b = 0; b < sizeof(T) / 4; ++b) reinterpret_cast<float*>(&v)[b] = 1.0f;
  GRID_STRIDE(i, count) dst[i] = v;
}
void launch_calibration(hipStream_t st, void* buf, int64_t bytes, double* out) {
  LAUNCH1D(k_cal_read<float>, st, bytes / 4, static_cast<const float*>(buf), bytes / 4, out);
  LAUNCH1D(k_cal_read<double>, st, bytes / 8, static_cast<const double*>(buf), bytes / 8, out);
  LAUNCH1D(k_cal_read<float4>, st, bytes / 16, static_cast<const float4*>(buf), bytes / 16, out);
  LAUNCH1D(k_cal_read<double4>, st, bytes / 32, static_cast<const double4*>(buf), bytes / 32, out);
  LAUNCH1D(k_cal_write<float>, st, bytes / 4, static_cast<float*>(buf), bytes / 4);
  LAUNCH1D(k_cal_write<double>, st, bytes / 8, static_cast<double*>(buf), bytes / 8);
  LAUNCH1D(k_cal_write<float4>, st, bytes / 16, static_cast<float4*>(buf), bytes / 16);
}

}  // namespace fsi
