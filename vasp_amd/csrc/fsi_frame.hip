// C-ABI of libvaspfsi.so (include/vaspfsi.h): one saved Visualization frame into the resident state (fsi_set_frame), so that
// the post-processing sessions of fsi_sessions.hip can run over a finished results folder.
//
// Replaces the read loop of vasp-create-hdf5 / create_transformed_matrix that rebuilds a Function from one saved frame
// [REF src/vasp/postprocessing/postprocessing_fenics/create_hdf5.py:139-160;
//  src/vasp/postprocessing/postprocessing_h5py/postprocessing_h5py_common.py:154-409].
//
// The frame's fields are staged in tmp7 in the user layout's places - d at 0, v at 3 N2, p at 6 N2 - which is the room of
// exactly one state vector (6 N2 + V doubles), in file order: [n_nodes][3] rows for d and v, the first V entries of p.
//
//   k_state_from_frame : one thread per user dof (node, component) of the fields that were given.  With n_nodes == N2 the
//                        staged entry is the dof's value; with n_nodes == V (save_deg 1) a vertex takes its row and a mid-edge
//                        node 0.5 * (a + b) of the edge's two vertex rows (edges[2 (node - V)], edges[2 (node - V) + 1]).
//                        Reads are coalesced in file order, the write goes to U[user2solver[dof]] as launch_scatter's does.
//                        Plain loads and stores, every solver entry written by one thread: no atomics.  256 threads per
//                        workgroup: the kernel has no reuse and no LDS, it only has to keep enough loads in flight.
#include "fsi_host.hpp"

#pragma clang fp contract(off)

using namespace fsi;
using namespace fsi::host;

namespace {

constexpr int FRAME_D = 1, FRAME_V = 2, FRAME_P = 4;

__global__ __launch_bounds__(256) void k_state_from_frame(int64_t N2, int64_t V, int64_t n_nodes, int fields,
                                                          const double* __restrict__ stage, const int32_t* __restrict__ edges,
                                                          const int32_t* __restrict__ user2solver, double* __restrict__ U) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nvec = 3 * N2;
  if (i >= 2 * nvec + V) return;
  double val;
  if (i >= 2 * nvec) {                       // pressure: the vertices, whatever the file's node count
    if (!(fields & FRAME_P)) return;
    val = stage[i];
  } else {
    const int f = i >= nvec ? 1 : 0;
    if (!(fields & (f ? FRAME_V : FRAME_D))) return;
    const int64_t off = f * nvec, j = i - off, node = j / 3;
    if (n_nodes == N2 || node < V) {
      val = stage[i];
    } else {
      const int comp = (int)(j - 3 * node);
      const int64_t a = edges[2 * (node - V)], b = edges[2 * (node - V) + 1];
      val = 0.5 * (stage[off + 3 * a + comp] + stage[off + 3 * b + comp]);
    }
  }
  U[user2solver[i]] = val;
}

// the two vertices of every mid-edge node, from the local P2 order of a tetrahedron: nodes 4 .. 9 are the edges (2,3), (1,3),
// (1,2), (0,3), (0,2), (0,1).  Built at the first save_deg 1 frame and kept for the life of the context.
int build_frame_edges(FsiCtx* ctx) {
  static const int EV[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
  const int64_t V = ctx->V, E = ctx->N2 - ctx->V;
  std::vector<int32_t> edges((size_t)(2 * E), -1);
  const int32_t* tn = ctx->h_tet_nodes.data();
  for (int64_t c = 0; c < ctx->C; ++c)
    for (int e = 0; e < 6; ++e) {
      const int64_t node = tn[10 * c + 4 + e], a = tn[10 * c + EV[e][0]], b = tn[10 * c + EV[e][1]];
      if (node < V || node >= ctx->N2 || a < 0 || a >= V || b < 0 || b >= V) {
        ctx->err = "fsi_set_frame: the mesh's P2 nodes are not vertices first, then one node per edge";
        return FSI_ERR_INVALID;
      }
      edges[2 * (node - V)] = (int32_t)a;
      edges[2 * (node - V) + 1] = (int32_t)b;
    }
  for (int32_t x : edges)
    if (x < 0) { ctx->err = "fsi_set_frame: a mid-edge node belongs to no cell"; return FSI_ERR_INVALID; }
  FSICHK(upload(ctx, ctx->frame_edges, edges));
  return FSI_OK;
}

double* frame_state(FsiCtx* ctx, int which) {
  switch (which) {
    case 0: return ctx->U.p;
    case 1: return ctx->U1.p;
    default: return nullptr;
  }
}

}  // namespace

int fsi_set_frame(FsiCtx* ctx, int which, int64_t n_nodes, const double* d, const double* v, const double* p) {
  if (!ctx) return FSI_ERR_INVALID;
  if (!frame_state(ctx, which)) { ctx->err = "fsi_set_frame: which must be 0 (dvp_[\"n\"]) or 1 (dvp_[\"n-1\"])"; return FSI_ERR_INVALID; }
  if (ctx->part) { ctx->err = "fsi_set_frame: partitioned contexts are not supported"; return FSI_ERR_INVALID; }
  const int64_t V = ctx->V, N2 = ctx->N2;
  if (n_nodes != V && n_nodes != N2) {
    ctx->err = "fsi_set_frame: a frame of " + std::to_string(n_nodes) + " nodes, the mesh has " + std::to_string(V) +
               " vertices (save_deg 1) and " + std::to_string(N2) + " P2 nodes (save_deg 2)";
    return FSI_ERR_INVALID;
  }
  const int fields = (d ? FRAME_D : 0) | (v ? FRAME_V : 0) | (p ? FRAME_P : 0);
  if (!fields) return FSI_OK;
  HIPCHK(hipSetDevice(ctx->device));
  if (n_nodes != N2 && (d || v) && !ctx->frame_edges.p && N2 > V) FSICHK(build_frame_edges(ctx));
  double* stage = ctx->tmp7.p;
  const size_t vec = (size_t)(3 * n_nodes) * sizeof(double);
  if (d) HIPCHK(hipMemcpyAsync(stage, d, vec, hipMemcpyHostToDevice, ctx->stream));
  if (v) HIPCHK(hipMemcpyAsync(stage + 3 * N2, v, vec, hipMemcpyHostToDevice, ctx->stream));
  if (p) HIPCHK(hipMemcpyAsync(stage + 6 * N2, p, (size_t)V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int64_t n = ctx->ndof;
  k_state_from_frame<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(N2, V, n_nodes, fields, stage, ctx->frame_edges.p,
                                                                                     ctx->user2solver.p, frame_state(ctx, which));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));          // the caller's views may be unmapped when the call returns
  return FSI_OK;
}
