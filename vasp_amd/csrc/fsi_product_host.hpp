// The host side of the monolithic product (MonoProduct, fsi_product.hpp) that needs no device: the forms a product can run in, the
// choice among them from what a Jacobian refresh found, and the layout arithmetic of the padded FP32 copy.  Plain C++: the
// library, the test shim and a stand-alone program read the same arithmetic.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fsi {

// How one product runs.  On the FP64 matrix: all six value rows of a node; the d rows from their pair form (six values per node
// pair); the d rows from the split pair form (three values per pair on a node without dv entries).  On the padded FP32 copy: six
// rows, or value rows 3 .. 5 with FP32 pair values.  (An FP32 split form does not exist.)
enum ProductForm : int { PRODUCT_SIX64 = 0, PRODUCT_PAIR64 = 1, PRODUCT_SPLIT64 = 2, PRODUCT_SIX32 = 3, PRODUCT_PAIR32 = 4 };
inline bool product_on_copy(ProductForm f) { return f == PRODUCT_SIX32 || f == PRODUCT_PAIR32; }
inline bool product_reads_pairs(ProductForm f) { return f != PRODUCT_SIX64 && f != PRODUCT_SIX32; }

// What a refresh decides, for the FP64 products and for those on the FP32 copy, until the next one.
//   pairs_ok       the extraction found nothing but dd_ii / dv_ii in the d rows of this matrix (compact_drows on, flag clear)
//   coupled_pairs  what the scan left in doff[N2]: the pairs of the nodes with dv entries (-1: not read); the split form is
//                  adopted when that fits the pair count of the node graph, and then holds 3 * coupled_pairs dv values
struct ProductForms {
  ProductForm f64 = PRODUCT_SIX64, f32 = PRODUCT_SIX32;
};
inline bool split_fits(bool pairs_ok, int64_t coupled_pairs, size_t npairs) {
  return pairs_ok && coupled_pairs >= 0 && (size_t)coupled_pairs <= npairs;
}
inline ProductForms choose_forms(bool pairs_ok, bool split_ok) {
  if (!pairs_ok) return {PRODUCT_SIX64, PRODUCT_SIX32};
  return {split_ok ? PRODUCT_SPLIT64 : PRODUCT_PAIR64, PRODUCT_PAIR32};
}

// The padded FP32 copy (k_spmv_node6p): the six value rows of a node, L entries each, padded to Lp = L rounded up to four, so that
// node r's block of 6 Lp values starts at entry p32[r] (a multiple of 24: float4 loads are aligned) and its index row of Lp
// entries at p32[r] / 6.  The pressure rows follow unpadded at entry ptail; they keep their own row pointers, which see the
// values through a shift.
struct PaddedTail {
  int64_t ptail = 0;         // first entry behind the padded node blocks = 6 * (entries of the padded index rows)
  int64_t src = 0;           // first entry of the pressure rows in the matrix: rowptr[6 N2]
  int64_t nnz = 0;           // entries of the pressure rows
  int64_t shift() const { return ptail - src; }      // vals32[shift + rowptr[row]] is the first value of pressure row `row`
  int64_t entries() const { return ptail + nnz; }    // length of the copy
};
// rowptr [>= 6 N2 + 1] of the monolithic matrix with nnz entries; p32 [N2 + 1] is written
inline PaddedTail padded_layout(const std::vector<int64_t>& rowptr, int64_t N2, int64_t nnz, std::vector<int64_t>& p32) {
  p32.assign((size_t)N2 + 1, 0);
  for (int64_t r = 0; r < N2; ++r) {
    const int64_t L = rowptr[6 * (size_t)r + 1] - rowptr[6 * (size_t)r];
    p32[(size_t)r + 1] = p32[(size_t)r] + 6 * ((L + 3) & ~(int64_t)3);
  }
  PaddedTail t;
  t.ptail = p32[(size_t)N2];
  t.src = rowptr[6 * (size_t)N2];
  t.nnz = nnz - t.src;
  return t;
}

}  // namespace fsi
