// One lane per listed cell of a recorded P2 vector history: what k_cell_rate, k_cell_rate_current (fsi_rate.hip),
// k_cell_vortex and k_cell_vortex_current (fsi_vortex.hip) share.  Device code only, included by those two files and nothing else.
//
// A lane keeps its cell's ten row indices and twelve gradient values in registers (CellLane), gathers the ten nodes' triples
// of a frame (240 B) and forms G_t = grad w at a vertex t - the gradient of a P2 field is linear on the cell, so the four
// vertices determine it.  The expression is that of wss_dg1_cell (fsi_wss.hpp); that one, the stress kernels and
// fsi_assembly.hip compile it with floating-point contraction and have their bits pinned by their own tests, so they keep their
// copies.  Here contraction is off - the pragma stands in this header, for code above the including file's own pragma would
// otherwise be contracted -: the NumPy twin (hi_pass.vertex_gradients) rounds every product and every sum, and the device
// equals it bit for bit.  This is the only copy of the expression the twins are held to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

namespace fsi {

// the ends of local edge e (local node 4 + e): mesh.TET_EDGES
__device__ constexpr int kEdge[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};

// what a lane keeps across its frame loop: 3 * the row of each of the cell's ten nodes within a frame, and gl[a][j], the
// gradient of barycentric coordinate a (launch_cell_gradients)
struct CellLane {
  int64_t row[10];
  double gl[4][3];
};

__device__ __forceinline__ void load_cell_lane(const int32_t* conn, const double* gl_all, int64_t c, CellLane& lane) {
#pragma unroll
  for (int a = 0; a < 10; ++a) lane.row[a] = 3 * (int64_t)conn[c * 10 + a];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 3; ++j) lane.gl[a][j] = gl_all[c * 12 + a * 3 + j];
}

// w[a][i]: component i of local node a in the frame that begins at f
__device__ __forceinline__ void gather_cell_frame(const double* f, const CellLane& lane, double (&w)[10][3]) {
#pragma unroll
  for (int a = 0; a < 10; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) w[a][i] = f[lane.row[a] + i];
}

// The products of the gradient values with the basis coefficients in vertex_gradient_of do not depend on the frame: left
// alone, the compiler forms all 78 of them once and keeps them in registers across the frame loop (k_cell_rate: 256 VGPRs +
// 68 AGPRs, one wave per SIMD).  Making gl opaque before each vertex has them formed again per vertex and frame - a quarter
// more multiplications, the same bits - and leaves k_cell_rate room for two waves per SIMD, which the gather needs to hide its
// latency.
__device__ __forceinline__ void fence_cell_gradients(double (&gl)[4][3]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(gl[a][j]));
}

// a vertex's nine values are done before the next vertex begins: left to the scheduler, the independent products of all four
// vertices are formed ahead of their sums (k_cell_rate_current: all 512 registers and 332 bytes of scratch per lane)
__device__ __forceinline__ void fence_vertex_gradient(double (&G)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) asm volatile("" : "+v"(G[i][j]));
}

// G = grad w at vertex t.  Every operation in the order of hi_pass.vertex_gradients.
__device__ __forceinline__ void vertex_gradient_of(const double (&w)[10][3], const double (&gl)[4][3], int t, double (&G)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) s = s + w[a][i] * ((a == t ? 3.0 : -1.0) * gl[a][j]);
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const int p = kEdge[e][0], r = kEdge[e][1];
        s = s + (w[4 + e][i] * 4.0) * ((p == t ? 1.0 : 0.0) * gl[r][j] + (r == t ? 1.0 : 0.0) * gl[p][j]);
      }
      G[i][j] = s;
    }
}

// G[t] = grad w at the four vertices t, one vertex after the other (the two fences above): what the kernels of the current
// configuration keep of a frame of the field and of the displacement
__device__ __forceinline__ void vertex_gradients_of(const double (&w)[10][3], double (&gl)[4][3], double (&G)[4][3][3]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    fence_cell_gradients(gl);
    vertex_gradient_of(w, gl, t, G[t]);
    fence_vertex_gradient(G[t]);
  }
}

}  // namespace fsi
