// Stand-alone check of the device-free arithmetic of the monolithic product (vasp_amd/csrc/fsi_product_host.hpp): the choice of
// forms over every verdict a refresh can read, and the padded layout of a few row-length lists - L = 0, every L % 4, rows past 256
// entries, no node rows, no pressure rows.  tests/test_product_host.py builds and runs it as it is.  By hand, on a machine without
// a GPU, from the repository root:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ivasp_amd/csrc tests/product_host_check.cpp
//       -o /tmp/product_host_check && /tmp/product_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fsi_product_host.hpp"

using namespace fsi;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void forms() {
  for (int pairs_ok = 0; pairs_ok < 2; ++pairs_ok)
    for (long long coupled : {-1LL, 0LL, 1LL, 9LL, 10LL, 11LL}) {
      const size_t npairs = 10;
      const bool split = split_fits(pairs_ok != 0, coupled, npairs);
      CHECK(split == (pairs_ok && coupled >= 0 && coupled <= 10));
      const ProductForms f = choose_forms(pairs_ok != 0, split);
      CHECK(f.f64 == (!pairs_ok ? PRODUCT_SIX64 : split ? PRODUCT_SPLIT64 : PRODUCT_PAIR64));
      CHECK(f.f32 == (pairs_ok ? PRODUCT_PAIR32 : PRODUCT_SIX32));
      CHECK(!product_on_copy(f.f64) && product_on_copy(f.f32));
      CHECK(product_reads_pairs(f.f64) == (pairs_ok != 0) && product_reads_pairs(f.f32) == (pairs_ok != 0));
    }
  const ProductForms none;
  CHECK(none.f64 == PRODUCT_SIX64 && none.f32 == PRODUCT_SIX32);
}

// node row lengths L (six rows each) and pressure row lengths P
static void layout(const std::vector<int64_t>& L, const std::vector<int64_t>& P) {
  const int64_t N2 = (int64_t)L.size();
  std::vector<int64_t> rowptr(1, 0);
  for (int64_t l : L)
    for (int k = 0; k < 6; ++k) rowptr.push_back(rowptr.back() + l);
  for (int64_t p : P) rowptr.push_back(rowptr.back() + p);
  const int64_t nnz = rowptr.back();
  std::vector<int64_t> p32(3, -7);      // resized by the call
  const PaddedTail t = padded_layout(rowptr, N2, nnz, p32);
  CHECK((int64_t)p32.size() == N2 + 1 && p32[0] == 0);
  int64_t pressure = 0;
  for (int64_t p : P) pressure += p;
  CHECK(t.src == rowptr[6 * (size_t)N2] && t.nnz == pressure && t.ptail == p32[(size_t)N2] && t.entries() == t.ptail + pressure);
  std::vector<char> owner((size_t)t.entries(), 0);      // every entry of the copy belongs to exactly one row
  for (int64_t r = 0; r < N2; ++r) {
    const int64_t Lp = (p32[(size_t)r + 1] - p32[(size_t)r]) / 6;
    CHECK(Lp % 4 == 0 && Lp >= L[(size_t)r] && Lp < L[(size_t)r] + 4 && p32[(size_t)r] % 24 == 0);
    for (int64_t e = p32[(size_t)r]; e < p32[(size_t)r + 1]; ++e) owner[(size_t)e] += 1;
  }
  for (size_t q = 0; q < P.size(); ++q)      // a pressure row keeps its own pointers: the copy's entry is shift + rowptr
    for (int64_t e = rowptr[6 * (size_t)N2 + q]; e < rowptr[6 * (size_t)N2 + q + 1]; ++e) {
      CHECK(t.shift() + e >= t.ptail && t.shift() + e < t.entries());
      owner[(size_t)(t.shift() + e)] += 1;
    }
  for (char c : owner) CHECK(c == 1);
}

int main() {
  forms();
  layout({}, {});
  layout({}, {3, 0, 5});
  layout({0}, {});
  layout({0, 1, 2, 3, 4, 5, 6, 7, 8}, {2, 0, 9});
  layout({255, 256, 257, 1023, 0, 0, 13}, {1});
  std::vector<int64_t> many;
  for (int i = 0; i < 1000; ++i) many.push_back((i * 37) % 301);
  layout(many, std::vector<int64_t>(333, 7));
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
