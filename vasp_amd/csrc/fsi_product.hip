// The product y = A x with the row-equilibrated monolithic Jacobian, which runs in every Krylov iteration: the generic CSR kernel,
// the node-row kernels in their five forms with the pressure rows behind them, the kernels that build the forms at a Jacobian
// refresh (pair and split form of the d rows, the padded FP32 copy), one launch function for a product, and MonoProduct, the
// context's operator (fsi_product.hpp; its device-free arithmetic in fsi_product_host.hpp).  HBM-bound; algorithmic bytes of a
// generic product: nnz * (8 + 4) + n * (8 + 8) + (n + 1) * 8.
#include "fsi_host.hpp"

namespace fsi {

// ---------------------------------------------------------------------------------------------------------
// SpMV, one wave per row (rows have ~100-400 entries)
// ---------------------------------------------------------------------------------------------------------
// TAG only names the instantiation (profiles list the monolithic, solid-block and other-block products separately)
template <int TAG, class VT = double>
__global__ __launch_bounds__(256) void k_spmv(int64_t n, const int64_t* __restrict__ rowptr,
                                              const int32_t* __restrict__ cols, const VT* __restrict__ vals,
                                              const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < n; row += nwaves) {
    const int64_t s = rowptr[row], e = rowptr[row + 1];
    double sum = 0.0;
    for (int64_t t = s + lane; t < e; t += 64) sum += (double)vals[t] * x[cols[t]];
    sum = wave_sum_dpp(sum);
    if (lane == 0) y[row] = sum;
  }
}
void launch_spmv(hipStream_t st, int64_t n, const int64_t* rowptr, const int32_t* cols, const double* vals,
                 const double* x, double* y, int tag) {
  if (n <= 0) return;      // no rows (an empty grid is an invalid launch)
  int64_t blocks = (n + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  if (tag == SPMV_MONOLITHIC)
    hipLaunchKernelGGL(k_spmv<SPMV_MONOLITHIC>, dim3((unsigned)blocks), dim3(256), 0, st, n, rowptr, cols, vals, x, y);
  else if (tag == SPMV_SOLID_BLOCK)
    hipLaunchKernelGGL(k_spmv<SPMV_SOLID_BLOCK>, dim3((unsigned)blocks), dim3(256), 0, st, n, rowptr, cols, vals, x, y);
  else
    hipLaunchKernelGGL(k_spmv<SPMV_FIELD_BLOCK>, dim3((unsigned)blocks), dim3(256), 0, st, n, rowptr, cols, vals, x, y);
}

// ---------------------------------------------------------------------------------------------------------
// The node rows.  The six rows of a node share their column pattern (k_expand_cols), so one wave takes a node, reads the column
// indices and gathers x ONCE and streams the six value rows against them - 8 + 4/6 instead of 12 bytes per entry, a sixth of the
// gathers, and six independent value streams in flight per lane.  The kernels below are made of five pieces, each written once:
// the nodes a wave takes, value rows against one row of column indices in the matrix's own layout and in the padded one, the d rows
// from their pair and split form, and the reduction of the six sums.  The accumulation order of every piece is part of its
// contract (tests/test_gpu_product_bits.py holds the bits).
// ---------------------------------------------------------------------------------------------------------
// The nodes of wave `wid` of this workgroup: first, first + stride, ... below last.
// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2; giving XCD k the k-th eighth of the
// nodes (instead of every eighth workgroup of one sweep over all nodes) keeps the x entries a node's neighbours gather
// inside ONE L2 instead of fetching them into all eight: -9 % HBM traffic (round 2).  It is the only mapping there is: the
// kernels keep their template argument XCD = true because profiles and tools know them by the names that carry it.
// One wave per node, no grid-stride loop (node_grid): measured 1.87 ms per product against 2.23 ms with 8192 workgroups looping
// (row lengths differ by 3x between edge and vertex nodes; the hardware scheduler balances what a static stride cannot).
// (waves = blockDim.x >> 6 and blocks = gridDim.x come from the kernel's own body: read inside a device function, blockDim.x is
// not folded to the scalar load of a uniform launch but fetched with a vector load at the start of every wave.)
struct WaveNodes {
  int64_t first, last, stride;
};
__device__ __forceinline__ WaveNodes wave_nodes(int64_t N2, int64_t wid, unsigned waves, unsigned blocks) {
  WaveNodes w;                                                  // blocks is a multiple of 8
  const int64_t chunk = (N2 + 7) >> 3, k = blockIdx.x & 7;
  w.first = k * chunk + (blockIdx.x >> 3) * (int64_t)waves + wid;
  w.last = (k + 1) * chunk < N2 ? (k + 1) * chunk : N2;
  w.stride = (int64_t)(blocks >> 3) * waves;
  return w;
}
// four nodes per workgroup, a multiple of 8 workgroups
static inline unsigned node_grid(int64_t N2) { return (unsigned)(((N2 + 3) / 4 + 7) & ~(int64_t)7); }
// The wave's index, made wave-uniform for the compiler (readfirstlane) so that the row and graph pointers of its node come through
// the scalar cache: this took the pair form from 2.27 / 1.67 ms per product (FP64 / FP32 copy, 1.12 M tets) to 2.14 / 1.58.  The
// two six-row kernels take it from threadIdx.x >> 6 as they always have.
__device__ inline int uniform_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// a_k += sum over the lane's entries t of v[k L + t] * x[c[t]] for the k-th of the accumulators given: as many value rows of L
// entries, back to back, against one row of column indices.  VT = float: an FP32 copy of the (row-equilibrated, |entries| <= 1)
// values; x, y and the accumulation stay FP64.  (The accumulators are separate doubles, not an array: the compiler keeps an array of
// six in one twelve-register tuple, two VGPRs more in every kernel.)
template <class VT, class... Acc>
__device__ __forceinline__ void rows_stream(const VT* __restrict__ v, const int32_t* __restrict__ c, int64_t L, int lane,
                                            const double* __restrict__ x, Acc&... a) {
  for (int64_t t = lane; t < L; t += 64) {
    const double xv = x[c[t]];
    int64_t k = 0;
    ((a += (double)v[k++ * L + t] * xv), ...);
  }
}
// The same on the padded FP32 copy (k_pad_cols32 / k_pad_vals32): rows of Lp entries, a multiple of four, 16-byte aligned.  One
// float4 / int4 load per lane covers 256 entries: the ~170 entries of a P2 edge node take ONE round of six + 1 loads and 4 gathers
// per lane instead of three rounds of 6 + 1 + 1 - the FP32 product was paced by its memory instructions, not by its 7.5 GB.
template <class... Acc>
__device__ __forceinline__ void rows_stream4(const float* __restrict__ v, const int32_t* __restrict__ c, int Lp, int lane,
                                             const double* __restrict__ x, Acc&... a) {
  for (int t = 4 * lane; t < Lp; t += 256) {
    const int4 cc = *reinterpret_cast<const int4*>(c + t);
    float4 w[sizeof...(Acc)];
#pragma unroll
    for (int k = 0; k < (int)sizeof...(Acc); ++k) w[k] = *reinterpret_cast<const float4*>(v + k * Lp + t);
    const double x0 = x[cc.x], x1 = x[cc.y], x2 = x[cc.z], x3 = x[cc.w];
    int k = 0;
    ((a += ((double)w[k].x * x0 + (double)w[k].y * x1) + ((double)w[k].z * x2 + (double)w[k].w * x3), ++k), ...);
  }
}
// the six sums of a node over the wave; lane 0 stores them
__device__ __forceinline__ void reduce_store6(double a0, double a1, double a2, double a3, double a4, double a5, int lane,
                                              double* __restrict__ o) {
  a0 = wave_sum_dpp(a0); a1 = wave_sum_dpp(a1); a2 = wave_sum_dpp(a2); a3 = wave_sum_dpp(a3); a4 = wave_sum_dpp(a4); a5 = wave_sum_dpp(a5);
  if (lane == 0) { o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4; o[5] = a5; }
}

// ---- displacement rows in pair form (round 5) -------------------------------------------------------------------------------
// The three d rows of a node hold 6 deg + pdeg entries each, of which at most 2 deg are structurally non-zero for the forms VaSP
// uses: the mesh-extension Laplacian and the solid's d - v relation act per component, so row (r, i) has dd_ii and dv_ii per
// neighbour and no pressure entry - 18 of the 36 values of a node pair carry 6 numbers.  k_drows_extract copies those six per
// pair [dd_0 dd_1 dd_2 dv_0 dv_1 dv_2] at every Jacobian refresh AND checks that every other entry of the d rows is exactly zero
// (flag bit 0 otherwise: the full product stays).  The products then stream the three v rows as before and take the d rows
// from the pair array with one lane per neighbour (48 contiguous bytes of values against the 48 contiguous bytes of x of that
// neighbour): 24 deg + 3 pdeg values + 6 deg pair values per node instead of 36 deg + 6 pdeg.
// (Round 2's "compact node rows" re-laid ALL 24 non-zeros as 24 short runs per node and was latency-bound: 3.46 against 3.20 ms.
// Here the v rows keep their three long streams.)
// The split form (dd != nullptr; FP64 products): A_dv has entries in the rows of solid nodes only, so on a fluid node - nine in ten
// on the bench mesh - the dv half of every pair is three exact zeros.  The kernel also writes dd [pairs][3] and classifies each node
// FROM THE VALUES IT READS: cdeg[r] = its degree if any dv entry of its three d rows is non-zero ("coupled"), else 0.  A scan turns
// cdeg into offsets (k_drows_offsets: doff[r] = first pair of r in dv, -1 for an uncoupled node) and k_drows_gather_dv copies the dv
// halves of the coupled nodes to dv [coupled pairs][3].  k_spmv_node6s then reads 24 bytes per pair on an uncoupled node instead of 48.
template <class DT>
__global__ __launch_bounds__(256) void k_drows_extract(int64_t N2, const int64_t* __restrict__ rowptr, const double* __restrict__ A,
                                                       const int64_t* __restrict__ nadj_ptr, double* __restrict__ ad64,
                                                       DT* __restrict__ ad32, int32_t* __restrict__ flag, double* __restrict__ dd,
                                                       int32_t* __restrict__ cdeg) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  bool bad = false;
  for (int64_t r = wave; r < N2; r += nwaves) {
    const int64_t s0 = rowptr[6 * r], L = rowptr[6 * r + 1] - s0, a = nadj_ptr[r], deg6 = 6 * (nadj_ptr[r + 1] - a);
    bool coupled = false;
    for (int i = 0; i < 3; ++i)
      for (int64_t t = lane; t < L; t += 64) {
        const double v = A[s0 + i * L + t];
        const int c = (int)(t % 6);
        if (t < deg6 && (c == i || c == i + 3)) {
          const int64_t o = 6 * (a + t / 6) + (c == i ? i : 3 + i);
          ad64[o] = v;
          if (ad32) ad32[o] = (DT)v;
          if (dd && c == i) dd[3 * (a + t / 6) + i] = v;
          if (c != i && v != 0.0) coupled = true;
        } else if (v != 0.0) bad = true;
      }
    if (cdeg) {                                                   // (r is the wave's: every lane is here)
      const bool any = __ballot(coupled) != 0;
      if (lane == 0) cdeg[r] = any ? (int32_t)(deg6 / 6) : 0;
    }
  }
  if (bad) atomicOr(flag, 1);
}
void launch_drows_extract_split(hipStream_t st, int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr,
                                double* ad64, float* ad32, int32_t* flag, double* dd, int32_t* cdeg) {
  int64_t blocks = std::min<int64_t>((N2 + 3) / 4, 16384);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_drows_extract<float>, dim3((unsigned)blocks), dim3(256), 0, st, N2, rowptr, A, nadj_ptr, ad64, ad32, flag, dd, cdeg);
}
void launch_drows_extract(hipStream_t st, int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr, double* ad64,
                          float* ad32, int32_t* flag) {
  launch_drows_extract_split(st, N2, rowptr, A, nadj_ptr, ad64, ad32, flag, nullptr, nullptr);
}
// doff[r] = sum of cdeg[0 .. r) where cdeg[r] > 0, else -1; doff[N2] = the whole sum.  One block: the scan runs once per Jacobian
// over one number per node, in tiles of 8192 nodes with the running sum carried along.
__global__ __launch_bounds__(1024) void k_drows_offsets(int64_t N2, const int32_t* __restrict__ cdeg, int64_t* __restrict__ doff) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t carry;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < N2; base += 8192) {              // eight consecutive nodes per thread
    const int64_t i0 = base + 8 * (int64_t)threadIdx.x;
    int32_t c[8];
    int64_t mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = i0 + j < N2 ? cdeg[i0 + j] : 0; mine += c[j]; }
    int64_t incl = mine;                                         // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int64_t before = carry;
    for (int k = 0; k < wv; ++k) before += wsum[k];
    int64_t at = before + incl - mine;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (i0 + j < N2) doff[i0 + j] = c[j] > 0 ? at : -1;
      at += c[j];
    }
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) doff[N2] = carry;
}
void launch_drows_offsets(hipStream_t st, int64_t N2, const int32_t* cdeg, int64_t* doff) {
  hipLaunchKernelGGL(k_drows_offsets, dim3(1), dim3(1024), 0, st, N2, cdeg, doff);
}
__global__ __launch_bounds__(256) void k_drows_gather_dv(int64_t N2, const int64_t* __restrict__ nadj_ptr, const int64_t* __restrict__ doff,
                                                         const double* __restrict__ ad64, double* __restrict__ dv) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < N2; r += nwaves) {
    const int64_t o = doff[r];
    if (o < 0) continue;
    const int64_t a = nadj_ptr[r], deg = nadj_ptr[r + 1] - a;
    for (int64_t t = lane; t < 3 * deg; t += 64) dv[3 * o + t] = ad64[6 * (a + t / 3) + 3 + t % 3];
  }
}
void launch_drows_gather_dv(hipStream_t st, int64_t N2, const int64_t* nadj_ptr, const int64_t* doff, const double* ad64, double* dv) {
  int64_t blocks = std::min<int64_t>((N2 + 3) / 4, 16384);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_drows_gather_dv, dim3((unsigned)blocks), dim3(256), 0, st, N2, nadj_ptr, doff, ad64, dv);
}
// the d rows of node r from the pair array: lane k takes neighbour k (AT: double | float)
template <class AT>
__device__ inline void drows_pairs(const AT* __restrict__ ad, const int32_t* __restrict__ nadj, int64_t a, int64_t deg, int lane,
                                   const double* __restrict__ x, double& a0, double& a1, double& a2) {
  for (int64_t k = lane; k < deg; k += 64) {
    const double2* xp = reinterpret_cast<const double2*>(x + 6 * (int64_t)nadj[a + k]);
    double d0, d1, d2, v0, v1, v2;
    if (sizeof(AT) == 8) {
      const double2* p = reinterpret_cast<const double2*>(ad + 6 * (a + k));
      const double2 p0 = p[0], p1 = p[1], p2 = p[2];
      d0 = p0.x; d1 = p0.y; d2 = p1.x; v0 = p1.y; v1 = p2.x; v2 = p2.y;
    } else {
      const float2* p = reinterpret_cast<const float2*>(ad + 6 * (a + k));
      const float2 p0 = p[0], p1 = p[1], p2 = p[2];
      d0 = p0.x; d1 = p0.y; d2 = p1.x; v0 = p1.y; v1 = p2.x; v2 = p2.y;
    }
    const double2 x0 = xp[0], x1 = xp[1], x2 = xp[2];      // d_x d_y | d_z v_x | v_y v_z of the neighbour
    a0 += d0 * x0.x + v0 * x1.y;
    a1 += d1 * x0.y + v1 * x2.x;
    a2 += d2 * x1.x + v2 * x2.y;
  }
}
// The d rows of node r from the split pair form (k_drows_extract with dd): o = doff[r] is wave-uniform.  What the six-value form
// computes per pair is  t = fma(d, x_d, v * x_v)  and then  a + t  (the ISA of drows_pairs: v_mul_f64, v_fma_f64, v_add_f64 - the sum
// of two products contracts to one FMA, the accumulation cannot).  With v == 0 that t is the ROUNDED product d * x_d, so the
// uncoupled node does one multiply and one add, kept apart (an FMA into the accumulator would round once instead of twice); the
// coupled node spells the same three operations out.  The results are those of drows_pairs bit for bit: an accumulator that starts
// as +0 never becomes -0, so not even the sign of the zero  v * x_v  shows.
__device__ inline void drows_split(const double* __restrict__ dd, const double* __restrict__ dv, int64_t o,
                                   const int32_t* __restrict__ nadj, int64_t a, int64_t deg, int lane,
                                   const double* __restrict__ x, double& a0, double& a1, double& a2) {
#pragma clang fp contract(off)
  if (o < 0) {
    for (int64_t k = lane; k < deg; k += 64) {
      const double* xp = x + 6 * (int64_t)nadj[a + k];
      const double* p = dd + 3 * (a + k);
      const double d0 = p[0], d1 = p[1], d2 = p[2];
      const double2 x0 = *reinterpret_cast<const double2*>(xp);      // d_x d_y | d_z of the neighbour
      const double x2 = xp[2];
      const double t0 = d0 * x0.x, t1 = d1 * x0.y, t2 = d2 * x2;
      a0 = a0 + t0; a1 = a1 + t1; a2 = a2 + t2;
    }
  } else {
    for (int64_t k = lane; k < deg; k += 64) {
      const double2* xp = reinterpret_cast<const double2*>(x + 6 * (int64_t)nadj[a + k]);
      const double* p = dd + 3 * (a + k);
      const double* q = dv + 3 * (o + k);
      const double d0 = p[0], d1 = p[1], d2 = p[2], v0 = q[0], v1 = q[1], v2 = q[2];
      const double2 x0 = xp[0], x1 = xp[1], x2 = xp[2];      // d_x d_y | d_z v_x | v_y v_z of the neighbour
      const double t0 = __builtin_fma(d0, x0.x, v0 * x1.y), t1 = __builtin_fma(d1, x0.y, v1 * x2.x), t2 = __builtin_fma(d2, x1.x, v2 * x2.y);
      a0 = a0 + t0; a1 = a1 + t1; a2 = a2 + t2;
    }
  }
}

// ---- the five node-row kernels: which pieces each is made of ---------------------------------------------------------------------
// all six value rows of the matrix (VT = float: of an FP32 copy in the matrix's own layout)
template <class VT, bool XCD>
__global__ __launch_bounds__(256) void k_spmv_node6(int64_t N2, const int64_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ cols, const VT* __restrict__ vals,
                                                    const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const WaveNodes w = wave_nodes(N2, threadIdx.x >> 6, blockDim.x >> 6, gridDim.x);
  for (int64_t r = w.first; r < w.last; r += w.stride) {
    const int64_t s0 = rowptr[6 * r];
    const int64_t L = rowptr[6 * r + 1] - s0;                  // the six rows are stored back to back with equal lengths
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    rows_stream(vals + s0, cols + s0, L, lane, x, a0, a1, a2, a3, a4, a5);
    reduce_store6(a0, a1, a2, a3, a4, a5, lane, y + 6 * r);
  }
}
// the d rows in pair form, value rows 3 .. 5 of the node's block only.
// (Also measured at 1.12 M tets, FP64 / FP32 copy, ms per product; this form 2.27 / 1.67, all six rows 2.56 - 2.72 / 1.73 - 1.82:
// the v rows taken neighbour by neighbour like the d rows - no column indices, x gathered once per neighbour, 48 contiguous bytes
// per lane and row - 2.27 / 1.93: 45 % of the lanes idle on a 29-neighbour node, 90 - 100 VGPRs; four strips of 64 entries issued
// together, a 182-entry row in one round of index -> gather: 2.45, two strips: 2.14 (the same): the product wants many small waves,
// not deep ones.)
template <bool XCD>
__global__ __launch_bounds__(256) void k_spmv_node6c(int64_t N2, const int64_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                     const int64_t* __restrict__ nadj_ptr, const int32_t* __restrict__ nadj,
                                                     const double* __restrict__ ad, const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const WaveNodes w = wave_nodes(N2, uniform_wave(), blockDim.x >> 6, gridDim.x);
  for (int64_t r = w.first; r < w.last; r += w.stride) {
    const int64_t s0 = rowptr[6 * r];
    const int64_t L = rowptr[6 * r + 1] - s0;
    const int64_t n0 = nadj_ptr[r], deg = nadj_ptr[r + 1] - n0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    drows_pairs<double>(ad, nadj, n0, deg, lane, x, a0, a1, a2);
    rows_stream(vals + s0 + 3 * L, cols + s0, L, lane, x, a3, a4, a5);
    reduce_store6(a0, a1, a2, a3, a4, a5, lane, y + 6 * r);
  }
}
// k_spmv_node6c with the d rows from the split pair form; everything else as there
template <bool XCD>
__global__ __launch_bounds__(256) void k_spmv_node6s(int64_t N2, const int64_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                     const int64_t* __restrict__ nadj_ptr, const int32_t* __restrict__ nadj,
                                                     const double* __restrict__ dd, const double* __restrict__ dv,
                                                     const int64_t* __restrict__ doff, const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const WaveNodes w = wave_nodes(N2, uniform_wave(), blockDim.x >> 6, gridDim.x);
  for (int64_t r = w.first; r < w.last; r += w.stride) {
    const int64_t s0 = rowptr[6 * r];
    const int64_t L = rowptr[6 * r + 1] - s0;
    const int64_t n0 = nadj_ptr[r], deg = nadj_ptr[r + 1] - n0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    drows_split(dd, dv, doff[r], nadj, n0, deg, lane, x, a0, a1, a2);
    rows_stream(vals + s0 + 3 * L, cols + s0, L, lane, x, a3, a4, a5);
    reduce_store6(a0, a1, a2, a3, a4, a5, lane, y + 6 * r);
  }
}
// all six value rows of the padded FP32 copy: node r's block of 6 Lp values at p32[r], its index row at p32[r] / 6
template <bool XCD>
__global__ __launch_bounds__(256) void k_spmv_node6p(int64_t N2, const int64_t* __restrict__ p32, const int32_t* __restrict__ cols32,
                                                     const float* __restrict__ vals, const double* __restrict__ x,
                                                     double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const WaveNodes w = wave_nodes(N2, threadIdx.x >> 6, blockDim.x >> 6, gridDim.x);
  for (int64_t r = w.first; r < w.last; r += w.stride) {
    const int64_t o = p32[r];
    const int Lp = (int)((p32[r + 1] - o) / 6);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    rows_stream4(vals + o, cols32 + o / 6, Lp, lane, x, a0, a1, a2, a3, a4, a5);
    reduce_store6(a0, a1, a2, a3, a4, a5, lane, y + 6 * r);
  }
}
// k_spmv_node6p with the d rows in pair form (FP32 pair values): value rows 3 .. 5 of the padded block only
template <bool XCD>
__global__ __launch_bounds__(256) void k_spmv_node6pc(int64_t N2, const int64_t* __restrict__ p32, const int32_t* __restrict__ cols32,
                                                      const float* __restrict__ vals, const int64_t* __restrict__ nadj_ptr,
                                                      const int32_t* __restrict__ nadj, const float* __restrict__ ad,
                                                      const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const WaveNodes w = wave_nodes(N2, uniform_wave(), blockDim.x >> 6, gridDim.x);
  for (int64_t r = w.first; r < w.last; r += w.stride) {
    const int64_t o = p32[r];
    const int Lp = (int)((p32[r + 1] - o) / 6);
    const int64_t n0 = nadj_ptr[r], deg = nadj_ptr[r + 1] - n0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
    drows_pairs<float>(ad, nadj, n0, deg, lane, x, a0, a1, a2);
    rows_stream4(vals + o + 3 * (int64_t)Lp, cols32 + o / 6, Lp, lane, x, a3, a4, a5);
    reduce_store6(a0, a1, a2, a3, a4, a5, lane, y + 6 * r);
  }
}

// Monolithic SpMV, pressure rows.  The row of vertex q (node rank r = vrank[q]) holds, for every neighbour node s of r in
// ascending order, the six columns 6 s .. 6 s + 5, then the pressure columns (k_expand_cols): a lane takes a neighbour, reads
// its rank from the node graph (4 bytes instead of six column indices), the six values and the six x entries - 48 contiguous,
// 16-byte aligned bytes - and the pressure part follows entry by entry.  One wave per row.  (The generic kernel this replaces
// read 12 bytes per entry and gathered x entry by entry: 222 us of a 1.53 ms product at 1.12 M tets.)
template <class VT>
__global__ __launch_bounds__(256) void k_spmv_prow(int64_t V, const int64_t* __restrict__ prowptr, const int32_t* __restrict__ cols,
                                                   const VT* __restrict__ vals, const int32_t* __restrict__ vrank,
                                                   const int64_t* __restrict__ nadj_ptr, const int32_t* __restrict__ nadj,
                                                   const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  // (wave-uniform for the compiler: the row's three levels of pointers - row, node rank, node graph - come through the scalar cache)
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + uniform_wave();
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t q = wave; q < V; q += nwaves) {
    const int64_t s = prowptr[q], e = prowptr[q + 1];
    const int32_t r = vrank[q];
    const int64_t a = nadj_ptr[r], deg = nadj_ptr[r + 1] - a;
    double sum = 0.0;
    for (int64_t k = lane; k < deg; k += 64) {
      const double2* xp = reinterpret_cast<const double2*>(x + 6 * (int64_t)nadj[a + k]);
      const VT* v = vals + s + 6 * k;
      const double2 x0 = xp[0], x1 = xp[1], x2 = xp[2];
      sum += ((double)v[0] * x0.x + (double)v[1] * x0.y) + ((double)v[2] * x1.x + (double)v[3] * x1.y) + ((double)v[4] * x2.x + (double)v[5] * x2.y);
    }
    for (int64_t t = s + 6 * deg + lane; t < e; t += 64) sum += (double)vals[t] * x[cols[t]];
    sum = wave_sum_dpp(sum);
    if (lane == 0) y[q] = sum;
  }
}
// vals: indexed by the rows' own pointers (for the FP32 copy: shifted so that vals[rowptr[row]] is the row's first value)
template <class VT>
static void spmv_prows(hipStream_t st, const ProductView& m, const VT* vals, const double* x, double* y) {
  if (m.V <= 0) return;
  const dim3 grid((unsigned)((m.V + 3) / 4)), block(256);
  const int64_t* prowptr = m.rowptr + 6 * m.N2;
  if (m.g.vrank && m.g.nadj_ptr && m.g.nadj)
    hipLaunchKernelGGL(k_spmv_prow<VT>, grid, block, 0, st, m.V, prowptr, m.cols, vals, m.g.vrank, m.g.nadj_ptr, m.g.nadj, x, y + 6 * m.N2);
  else      // no node graph at hand: the generic kernel on the tail of the matrix
    hipLaunchKernelGGL((k_spmv<SPMV_MONOLITHIC, VT>), grid, block, 0, st, m.V, prowptr, m.cols, vals, x, y + 6 * m.N2);
}
int launch_product(hipStream_t st, const ProductView& m, ProductForm form, const double* x, double* y) {
  if (product_reads_pairs(form) && (!m.g.nadj_ptr || !m.g.nadj)) return LAUNCH_REFUSED;
  if ((form == PRODUCT_PAIR64 && !m.ad64) || (form == PRODUCT_PAIR32 && !m.ad32)) return LAUNCH_REFUSED;
  if (form == PRODUCT_SPLIT64 && (!m.dd || !m.doff)) return LAUNCH_REFUSED;      // (dv may be null: no coupled node)
  const dim3 grid(node_grid(m.N2)), block(256);
  if (m.N2 > 0) switch (form) {      // (no node rows: an empty grid is an invalid launch)
    case PRODUCT_SIX64:
      hipLaunchKernelGGL((k_spmv_node6<double, true>), grid, block, 0, st, m.N2, m.rowptr, m.cols, m.vals, x, y);
      break;
    case PRODUCT_PAIR64:
      hipLaunchKernelGGL(k_spmv_node6c<true>, grid, block, 0, st, m.N2, m.rowptr, m.cols, m.vals, m.g.nadj_ptr, m.g.nadj, m.ad64, x, y);
      break;
    case PRODUCT_SPLIT64:
      hipLaunchKernelGGL(k_spmv_node6s<true>, grid, block, 0, st, m.N2, m.rowptr, m.cols, m.vals, m.g.nadj_ptr, m.g.nadj, m.dd, m.dv, m.doff, x, y);
      break;
    case PRODUCT_SIX32:
      hipLaunchKernelGGL(k_spmv_node6p<true>, grid, block, 0, st, m.N2, m.p32, m.cols32, m.vals32, x, y);
      break;
    case PRODUCT_PAIR32:
      hipLaunchKernelGGL(k_spmv_node6pc<true>, grid, block, 0, st, m.N2, m.p32, m.cols32, m.vals32, m.g.nadj_ptr, m.g.nadj, m.ad32, x, y);
      break;
  }
  if (product_on_copy(form)) spmv_prows<float>(st, m, m.vals32 + m.tail_shift, x, y);
  else spmv_prows<double>(st, m, m.vals, x, y);
  return 0;
}

// ---- FP32 copy of the Jacobian in its own layout --------------------------------------------------------------------
// The copy only serves k_spmv_node6p / k_spmv_node6pc, so it is laid out for them (PaddedTail, fsi_product_host.hpp): the six value
// rows of a node (and one row of column indices) padded to a multiple of four entries and 16-byte aligned, p32[r] = first entry
// of node r's block in units of ENTRIES (block = 6 Lp values; the index row has Lp entries at p32[r] / 6).  Padding entries carry
// value 0 and column 0.  The pressure rows follow unpadded.
__global__ __launch_bounds__(256) void k_pad_cols32(int64_t N2, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                    const int64_t* __restrict__ p32, int32_t* __restrict__ cols32) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < N2; r += nwaves) {
    const int64_t s0 = rowptr[6 * r], L = rowptr[6 * r + 1] - s0, Lp = (L + 3) & ~(int64_t)3, o = p32[r] / 6;
    for (int64_t t = lane; t < Lp; t += 64) cols32[o + t] = t < L ? cols[s0 + t] : 0;
  }
}
__global__ __launch_bounds__(256) void k_pad_vals32(int64_t N2, const int64_t* __restrict__ rowptr, const double* __restrict__ A,
                                                    const int64_t* __restrict__ p32, float* __restrict__ A32, int row0) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < N2; r += nwaves) {
    const int64_t s0 = rowptr[6 * r], L = rowptr[6 * r + 1] - s0, Lp = (L + 3) & ~(int64_t)3, o = p32[r];
    for (int k = row0; k < 6; ++k)
      for (int64_t t = lane; t < Lp; t += 64) A32[o + k * Lp + t] = t < L ? (float)A[s0 + k * L + t] : 0.f;
  }
}
__global__ __launch_bounds__(256) void k_round_to_f32(int64_t n, const double* __restrict__ a, float* __restrict__ b) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) b[i] = (float)a[i];
}
void launch_round_to_f32(hipStream_t st, int64_t n, const double* a, float* b) {
  if (n <= 0) return;      // nothing to round (an empty grid is an invalid launch)
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_round_to_f32, dim3((unsigned)blocks), dim3(256), 0, st, n, a, b);
}
void launch_pad_cols32(hipStream_t st, int64_t N2, const int64_t* rowptr, const int32_t* cols, const int64_t* p32, int32_t* cols32) {
  int64_t blocks = std::min<int64_t>((N2 + 3) / 4, 8192);
  if (blocks > 0) hipLaunchKernelGGL(k_pad_cols32, dim3((unsigned)blocks), dim3(256), 0, st, N2, rowptr, cols, p32, cols32);
}
// node rows padded (k_pad_vals32), pressure rows as they are behind them at entry offset ptail
void launch_pad_vals32(hipStream_t st, int64_t N2, int64_t V, const int64_t* rowptr, const double* A, const int64_t* p32,
                       int64_t ptail, int64_t nnz_tail, int64_t tail_src, float* A32, bool v_rows_only) {
  int64_t blocks = std::min<int64_t>((N2 + 3) / 4, 8192);
  if (blocks > 0) hipLaunchKernelGGL(k_pad_vals32, dim3((unsigned)blocks), dim3(256), 0, st, N2, rowptr, A, p32, A32, v_rows_only ? 3 : 0);
  if (V > 0 && nnz_tail > 0) launch_round_to_f32(st, nnz_tail, A + tail_src, A32 + ptail);
}

// ---- the context's operator -----------------------------------------------------------------------------------------------------
// produces: the FP32 copy's layout and index rows; the values follow at every refresh
int MonoProduct::layout(FsiCtx* ctx, const std::vector<int64_t>& rowptr) {
  std::vector<int64_t> p32;
  tail = padded_layout(rowptr, ctx->N2, ctx->nnz, p32);
  FSICHK(host::upload(ctx, a32_ptr, p32));
  HIPCHK(a32_cols.alloc((size_t)(tail.ptail / 6)));
  launch_pad_cols32(ctx->stream, ctx->N2, ctx->rowptr.p, ctx->cols.p, a32_ptr.p, a32_cols.p);
  HIPCHK(A32.alloc((size_t)tail.entries()));
  return FSI_OK;
}
int MonoProduct::refresh(FsiCtx* ctx) {
  copy_ok = false;
  const bool copy32 = policy32 && ctx->kry_fp32_policy != 0 && ctx->precond == 0 && A32.p;
  // the d rows in pair form for the outer products (FsiTuning.compact_drows): extracted from THIS matrix, and adopted only if the
  // kernel found nothing else in those rows (one flag read per refresh)
  form = ProductForms{};
  if (getenv("FSI_DEBUG_DROWS_INJECT") && ctx->nnz > 1) {
    // test hook: a value where the forms leave a structural zero - entry 1 of the first d row (column d_y of node 0's first
    // neighbour in a d_x row) - so that the check below has a matrix to refuse
    const int64_t pos = 1;
    const double val = 0.125;
    int64_t* dpos = reinterpret_cast<int64_t*>(ctx->scratch.p + 4098);
    HIPCHK(hipMemcpyAsync(dpos, &pos, sizeof pos, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->scratch.p + 4099, &val, sizeof val, hipMemcpyHostToDevice, ctx->stream));
    launch_add_at(ctx->stream, ctx->A.p, dpos, ctx->scratch.p + 4099, 1.0, 1);
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  if (ctx->tune.compact_drows && ctx->N2 > 0) {
    const size_t npairs6 = 6 * (size_t)ctx->nadj.n;
    if (!Ad64.p) HIPCHK(Ad64.alloc(npairs6));
    if (copy32 && !Ad32.p) HIPCHK(Ad32.alloc(npairs6));
    HIPCHK(hipMemsetAsync(ctx->iflags.p + FsiCtx::IFLAG_DROWS, 0, sizeof(int32_t), ctx->stream));
    // ... and split for the FP64 products: dd for every pair, the nodes classified by their dv values, offsets by a scan
    if (!Add.p) HIPCHK(Add.alloc(npairs6 / 2));
    if (!cdeg.p) HIPCHK(cdeg.alloc((size_t)ctx->N2));
    if (!doff.p) HIPCHK(doff.alloc((size_t)ctx->N2 + 1));
    launch_drows_extract_split(ctx->stream, ctx->N2, ctx->rowptr.p, ctx->A.p, ctx->nadj_ptr.p, Ad64.p, copy32 ? Ad32.p : nullptr,
                               ctx->iflags.p + FsiCtx::IFLAG_DROWS, Add.p, cdeg.p);
    launch_drows_offsets(ctx->stream, ctx->N2, cdeg.p, doff.p);
    int32_t found = 1;
    int64_t coupled_pairs = -1;
    HIPCHK(hipMemcpyAsync(&found, ctx->iflags.p + FsiCtx::IFLAG_DROWS, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&coupled_pairs, doff.p + ctx->N2, sizeof coupled_pairs, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const bool split_ok = split_fits(found == 0, coupled_pairs, ctx->nadj.n);
    if (split_ok) {
      if (3 * (size_t)coupled_pairs > Adv3.n) HIPCHK(Adv3.alloc(3 * (size_t)coupled_pairs));
      if (coupled_pairs > 0) launch_drows_gather_dv(ctx->stream, ctx->N2, ctx->nadj_ptr.p, doff.p, Ad64.p, Adv3.p);
    }
    form = choose_forms(found == 0, split_ok);
    if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] displacement rows of the outer product in pair form: %s; %lld of %lld pairs belong to nodes with dv entries\n",
                                     pairs() ? "yes" : "no (other entries found)", (long long)coupled_pairs, (long long)ctx->nadj.n);
  }
  if (copy32) {
    launch_pad_vals32(ctx->stream, ctx->N2, ctx->V, ctx->rowptr.p, ctx->A.p, a32_ptr.p, tail.ptail, tail.nnz, tail.src, A32.p,
                      pairs());       // rows are equilibrated: |entries| <= 1
    copy_ok = true;
  }
  return FSI_OK;
}
// working = true: the product inside a Krylov iteration, which may run on the FP32 copy of the matrix while the basis of this
// Jacobian's lifetime is kept in FP32 (see solve_gcr); every other product (true residuals, the other solvers) is FP64
int MonoProduct::apply(FsiCtx* ctx, const double* x, double* y, bool working) {
  const ProductForm f = working && copy_ok && ctx->kry_fp32 ? form.f32 : form.f64;
  ProductView m;
  m.N2 = ctx->N2; m.V = ctx->V; m.rowptr = ctx->rowptr.p; m.cols = ctx->cols.p; m.vals = ctx->A.p;
  m.g = PRowGraph{ctx->vrank.p, ctx->nadj_ptr.p, ctx->nadj.p};
  m.p32 = a32_ptr.p; m.cols32 = a32_cols.p; m.vals32 = A32.p; m.tail_shift = tail.shift();
  m.ad64 = Ad64.p; m.ad32 = Ad32.p; m.dd = Add.p; m.dv = Adv3.p; m.doff = doff.p;
  const int rc = launch_product(ctx->stream, m, f, x, y);
  if (rc != 0) return rc;
  if (product_on_copy(f)) products32 += 1;
  if (product_reads_pairs(f)) pair_products += 1;
  return 0;
}

}  // namespace fsi
