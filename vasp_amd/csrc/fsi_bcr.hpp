// Descriptors of the exact coarse solve by block cyclic reduction (fsi_bcr.hip), shared with the test shim
// (fsi_kernel_shim.hip), and the builders of their tile lists: the shim runs the kernels on exactly what bcr_plan emits.
#pragma once
#include <vector>

#include "fsi_context.hpp"

namespace fsi {

struct BcrSeg { int32_t off, len, src; };                    // input segment of a solve task: src 0 = b, 1 = x
struct BcrTask {                                             // out[rows] (+)= W[rows][ldw] . concat(segments)
  int64_t w;                                                 // offset of W in the FP32 arena
  int32_t rows, ldw, out, nseg;
  BcrSeg seg[3];
};
struct BcrTile { int32_t task, row0; };                      // 16 rows of a task: one workgroup
struct BcrGemm {                                             // C = beta C + alpha (A1 B1 + A2 B2), optional FP32 copy
  int64_t a1, b1, a2, b2, c, o32;
  int32_t M, N, K1, K2, lda1, ldb1, lda2, ldb2, ldc, ld32;
  double alpha, beta;
};
struct BcrGemmTile { int32_t task, ti, tj; };                // 64 x 64 tile of C: one workgroup
struct BcrInv {                                              // in-place inverse of an m x m block (+ FP32 copy)
  int64_t a, o32, cb, rb;                                    // cb [m][32], rb [32][m]: column / row panel scratch of the blocked Gauss-Jordan
  int32_t m, ld, ld32;
};
constexpr int BCR_PANEL = 32;

struct BcrRange { int64_t first = 0, count = 0; };
struct BcrLevelHost {
  BcrRange inv, invupd, gemm1, gemm2, fwd, bwd;            // invupd: tiles of the rank-32 updates A += -Cb Rb of the inverses
  int inv_maxm = 0, fwd_maxld = 0, bwd_maxld = 0;
};

struct BcrData {
  bool planned = false, ready = false;
  int64_t nc = 0, n = 0, K = 0;
  int max_block = 0;
  DevBuf<int32_t> pos;                                       // coarse node -> position in BFS-level order
  DevBuf<int64_t> fill_dst;                                  // per sparse 3x3 block: offset of its (0,0) entry in the FP64 arena
  DevBuf<int32_t> fill_ld;
  int64_t nfill = 0, level0_doubles = 0;
  DevBuf<double> arena64, b, x;
  DevBuf<float> arena32;
  DevBuf<BcrTask> tasks;
  DevBuf<BcrTile> tiles;
  DevBuf<BcrGemm> gemms;
  DevBuf<BcrGemmTile> gtiles;
  DevBuf<BcrInv> invs;
  DevBuf<int32_t> flag;                                      // device: bit 0 = a pivot vanished / an operator was not finite in FP32
  std::vector<BcrLevelHost> levels;
  BcrRange top_inv, top_invupd, top_task;
  int top_m = 0, top_ld = 0;
  int64_t bytes32 = 0, bytes64 = 0, setup_flops = 0;
  int launches_per_solve = 0;
};

// ---- tile lists (host) ------------------------------------------------------------------------------------------------------
// the 64 x 64 tiles of C of product `id`, row-tile major
inline void bcr_gemm_tiles(const BcrGemm& g, int32_t id, std::vector<BcrGemmTile>& out) {
  for (int ti = 0; ti < (g.M + 63) / 64; ++ti)
    for (int tj = 0; tj < (g.N + 63) / 64; ++tj) out.push_back(BcrGemmTile{id, ti, tj});
}
// the 16-row tiles of solve task `id`
inline void bcr_task_tiles(const BcrTask& t, int32_t id, std::vector<BcrTile>& out) {
  for (int r0 = 0; r0 < t.rows; r0 += 16) out.push_back(BcrTile{id, r0});
}
// an in-place inverse of the m x m block at D (leading dimension m) with its panel scratch cb [m][32], rb [32][m], and the
// rank-32 update A += -Cb Rb that follows every panel (run as one k_bcr_gemm per panel)
inline BcrInv bcr_inverse(int64_t D, int64_t o32, int64_t cb, int64_t rb, int m, int ld32) { return BcrInv{D, o32, cb, rb, m, m, ld32}; }
inline BcrGemm bcr_inverse_update(const BcrInv& v) {
  return BcrGemm{v.cb, v.rb, -1, -1, v.a, -1, v.m, v.m, BCR_PANEL, 0, BCR_PANEL, v.m, 0, 0, v.ld, 0, -1.0, 1.0};
}

}  // namespace fsi
