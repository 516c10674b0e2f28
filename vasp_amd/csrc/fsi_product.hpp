// The product y = A x with the row-equilibrated monolithic Jacobian (fsi_product.hip): its kernels' launch functions, the view of
// device pointers one product reads, and MonoProduct, the context's operator - the padded FP32 copy, the pair and split forms of the
// d rows, and which form each kind of product runs until the next Jacobian refresh.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "fsi_devbuf.hpp"
#include "fsi_product_host.hpp"

struct FsiCtx;

namespace fsi {

enum SpmvTag : int { SPMV_MONOLITHIC = 0, SPMV_SOLID_BLOCK = 1, SPMV_FIELD_BLOCK = 2 };
// generic CSR, one wave per row; the tag only names the instantiation in a profile
void launch_spmv(hipStream_t st, int64_t n, const int64_t* rowptr, const int32_t* cols, const double* vals,
                 const double* x, double* y, int tag = SPMV_FIELD_BLOCK);
void launch_round_to_f32(hipStream_t st, int64_t n, const double* a, float* b);
// the padded FP32 copy (PaddedTail, fsi_product_host.hpp): the index rows once per context, the values at every refresh
// (v_rows_only: the d rows are served from their pair form - k_spmv_node6pc never reads value rows 0 .. 2 of the copy)
void launch_pad_cols32(hipStream_t st, int64_t N2, const int64_t* rowptr, const int32_t* cols, const int64_t* p32, int32_t* cols32);
void launch_pad_vals32(hipStream_t st, int64_t N2, int64_t V, const int64_t* rowptr, const double* A, const int64_t* p32,
                       int64_t ptail, int64_t nnz_tail, int64_t tail_src, float* A32, bool v_rows_only = false);
// d rows of the node blocks in pair form [dd_0 dd_1 dd_2 dv_0 dv_1 dv_2] per node pair; flag bit 0: a d row holds something else
// and the products must keep the full rows
void launch_drows_extract(hipStream_t st, int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr, double* ad64,
                          float* ad32, int32_t* flag);
// The pair form split (FP64): dd [pairs][3] for every node and dv [pairs of coupled nodes][3], a node being coupled when any dv
// entry of its three d rows is not exactly zero - found from the values at every refresh, like the verdict in `flag`.
//   launch_drows_extract_split   launch_drows_extract, and dd and cdeg [N2]: the node's degree if it is coupled, else 0
//   launch_drows_offsets         doff [N2 + 1]: first pair of node r in dv, -1 for an uncoupled node; doff[N2] = pairs in dv
//   launch_drows_gather_dv       dv from the pair form ad64 through doff (dv holds at least doff[N2] pairs)
void launch_drows_extract_split(hipStream_t st, int64_t N2, const int64_t* rowptr, const double* A, const int64_t* nadj_ptr,
                                double* ad64, float* ad32, int32_t* flag, double* dd, int32_t* cdeg);
void launch_drows_offsets(hipStream_t st, int64_t N2, const int32_t* cdeg, int64_t* doff);
void launch_drows_gather_dv(hipStream_t st, int64_t N2, const int64_t* nadj_ptr, const int64_t* doff, const double* ad64, double* dv);

// the node graph the pressure rows of the monolithic matrix were laid out from (k_expand_cols): with it the products read one
// neighbour rank per six entries (k_spmv_prow); all null: the generic CSR kernel
struct PRowGraph {
  const int32_t* vrank = nullptr;
  const int64_t* nadj_ptr = nullptr;
  const int32_t* nadj = nullptr;
};
// What one product reads; a form leaves what it does not read null.
struct ProductView {
  int64_t N2 = 0, V = 0;
  const int64_t* rowptr = nullptr;      // the matrix: [6 N2 + V + 1], the six rows of a node back to back with equal lengths
  const int32_t* cols = nullptr;
  const double* vals = nullptr;
  PRowGraph g;
  const int64_t* p32 = nullptr;         // the padded FP32 copy: [N2 + 1] first entry of a node's block
  const int32_t* cols32 = nullptr;      // padded index rows
  const float* vals32 = nullptr;        // padded node blocks, then the pressure rows: their values at vals32 + tail_shift + rowptr[row]
  int64_t tail_shift = 0;
  const double* ad64 = nullptr;         // pair form [6 x node pairs], FP64 and rounded
  const float* ad32 = nullptr;
  const double* dd = nullptr;           // split form: [3 x node pairs], [3 x pairs of coupled nodes] (null: no coupled node), [N2 + 1]
  const double* dv = nullptr;
  const int64_t* doff = nullptr;
};
// y = A x in the given form: the node rows, then the pressure rows.  Status 0: launched.  LAUNCH_REFUSED: nothing launched - a
// pair or split form without the node graph that indexes it (the six-row kernel instead would read d rows that a pair-form copy need
// not hold), a pair form without its values, or the split form without dd / doff.
constexpr int LAUNCH_REFUSED = 2;
int launch_product(hipStream_t st, const ProductView& m, ProductForm form, const double* x, double* y);

// The context's monolithic operator beside the matrix itself (FsiCtx::A on rowptr / cols).  Every form is extracted from THE
// matrix of the last refresh and adopted only after a check of its values; the counters are those of fsi_get_timers.
struct MonoProduct {
  int policy32 = 1;                     // FsiTuning.operator_fp32: products inside Krylov iterations on the FP32 copy (with an FP32 basis)
  DevBuf<float> A32;                    // the copy, in its own layout; allocated by layout(), filled by refresh()
  DevBuf<int64_t> a32_ptr;              // [N2 + 1]
  DevBuf<int32_t> a32_cols;
  PaddedTail tail;
  bool copy_ok = false;                 // A32 holds the values of the present matrix
  // d rows in pair form (k_drows_extract: six values per node pair instead of 18 + pressure columns; FsiTuning.compact_drows)
  DevBuf<double> Ad64;                  // [6 x node pairs]
  DevBuf<float> Ad32;                   // ... rounded, for the products on the copy
  // ... and split for the FP64 products (k_spmv_node6s): dd for every pair, dv for the pairs of the nodes whose d rows hold a
  // non-zero dv entry (the solid's)
  DevBuf<double> Add, Adv3;             // [3 x node pairs], [3 x pairs of coupled nodes] (grows when a refresh finds more)
  DevBuf<int32_t> cdeg;                 // [N2] degree of a coupled node, 0 of an uncoupled one
  DevBuf<int64_t> doff;                 // [N2 + 1] first pair of a coupled node in Adv3, -1: uncoupled; [N2]: pairs in Adv3
  ProductForms form;                    // what refresh() chose
  int64_t products32 = 0;               // products run on the copy
  int64_t pair_products = 0;            // products that took the d rows from a pair form
  bool pairs() const { return product_reads_pairs(form.f64); }

  int layout(FsiCtx* ctx, const std::vector<int64_t>& rowptr);      // set-up: the copy's layout and index rows
  int refresh(FsiCtx* ctx);                                         // a new Jacobian in ctx->A: every form of it, and the choice
  int apply(FsiCtx* ctx, const double* x, double* y, bool working); // one product; status of launch_product
};

}  // namespace fsi
