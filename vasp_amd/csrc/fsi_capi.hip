// C-ABI of libvaspfsi.so (include/vaspfsi.h) after set-up (fsi_setup.hip): boundary data, partition, state access, products, probes, timers.
//
// Host-side logic follows turtleFSI's monolithic.py / newtonsolver.py as VaSP uses them; the
// arithmetic runs in the HIP kernels of fsi_assembly.hip / fsi_solver.hip.
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace fsi {
namespace host {

ElemArrays elem_arrays(FsiCtx* c) {
  return ElemArrays{c->geom.p, c->cell_dofs.p, c->cell_kind.p, c->cell_region.p, c->cell_rank.p, c->cell_prow.p, c->enbr.p, c->epnbr.p};
}
ResidualGather residual_gather(const FsiCtx* c) {
  ResidualGather rg;
  if (c->Re.p) { rg.Re = c->Re.p; rg.N2 = c->N2; rg.V = c->V; rg.inc_ptr = c->inc_ptr.p; rg.inc = c->inc.p; rg.pinc_ptr = c->pinc_ptr.p; rg.pinc = c->pinc.p; }
  return rg;
}
CellColours cell_colours(const FsiCtx* c) {
  CellColours cc;
  if (c->ncellcol > 0) { cc.ncolours = c->ncellcol; cc.cells = c->col_cells.p; cc.ptr = c->h_col_ptr.data(); }
  return cc;
}
ElemParams elem_params(FsiCtx* c) {
  ElemParams ep;
  ep.sc = c->scheme;
  for (int i = 0; i < MAX_REGIONS; ++i) { ep.fluid[i] = c->fluid[i]; ep.solid[i] = c->solid[i]; }
  return ep;
}

int host_scalar(FsiCtx* ctx, const double* dptr, double* out) {
  HIPCHK(hipMemcpyAsync(out, dptr, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}
int dot_n(FsiCtx* ctx, const double* x, const double* y, int64_t n, double* out) {
  launch_dot(ctx->stream, x, y, n, ctx->scratch.p, ctx->scratch.p + 4096);
  return host_scalar(ctx, ctx->scratch.p + 4096, out);
}
int dot(FsiCtx* ctx, const double* x, const double* y, double* out) { return dot_n(ctx, x, y, ctx->ndof, out); }
int norm2(FsiCtx* ctx, const double* x, double* out) {
  FSICHK(dot(ctx, x, x, out));
  *out = std::sqrt(*out);
  return FSI_OK;
}

// ---- element partition: sums over ranks, owner -> ghost refresh (fsi_set_partition) -----------------------------------
int allreduce(FsiCtx* ctx, double* v, int n) {
  if (!ctx->part) return FSI_OK;
  ctx->allreduce_calls += 1;
  if (ctx->rccl) return rccl_allreduce_host(ctx, v, n);
  if (ctx->comm.allreduce_sum(ctx->comm.user, v, n) != 0) { ctx->err = "allreduce callback failed"; return FSI_ERR_DEVICE; }
  return FSI_OK;
}
// Partitioned runs: a status decided from rank-local data (a preconditioner self-test, a pivot, a device error) must be
// the same on every rank before the next collective, or the job hangs in it.  Every rank calls this at the same points.
int agree(FsiCtx* ctx, int rc) {
  if (!ctx->part) return rc;
  double bad = rc == FSI_OK ? 0.0 : 1.0;
  if (ctx->rccl) { if (rccl_allreduce_host(ctx, &bad, 1) != FSI_OK) return FSI_ERR_DEVICE; }
  else if (ctx->comm.allreduce_sum(ctx->comm.user, &bad, 1) != 0) { ctx->err = "allreduce callback failed"; return FSI_ERR_DEVICE; }
  ctx->allreduce_calls += 1;
  if (rc == FSI_OK && bad > 0.0) { ctx->err = "another rank of the partitioned job reported an error"; return FSI_ERR_LINEAR; }
  return rc;
}
// dot / norm over all ranks; the operands carry zeros in their ghost entries, so the local sums add up
int gdot(FsiCtx* ctx, const double* x, const double* y, double* out) {
  FSICHK(dot(ctx, x, y, out));
  return allreduce(ctx, out, 1);
}
int gnorm2(FsiCtx* ctx, const double* x, double* out) {
  FSICHK(gdot(ctx, x, x, out));
  *out = std::sqrt(*out);
  return FSI_OK;
}
int halo_update(FsiCtx* ctx, double* x) {
  if (!ctx->part) return FSI_OK;
  ctx->halo_calls += 1;
  if (ctx->nsend) launch_gather(ctx->stream, ctx->sendbuf, x, ctx->send_idx.p, ctx->nsend);
  if (ctx->rccl) {      // pack -> grouped send / recv -> unpack, all on the solver stream: the host does not wait
    FSICHK(rccl_halo(ctx));
    if (ctx->nghost) launch_scatter(ctx->stream, x, ctx->recvbuf, ctx->ghost_idx.p, ctx->nghost);
    return FSI_OK;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->comm.halo_exchange(ctx->comm.user) != 0) { ctx->err = "halo_exchange callback failed"; return FSI_ERR_DEVICE; }
  if (ctx->nghost) launch_scatter(ctx->stream, x, ctx->recvbuf, ctx->ghost_idx.p, ctx->nghost);
  return FSI_OK;
}
void zero_ghost(FsiCtx* ctx, double* x) {
  if (ctx->part && ctx->nghost) launch_bc_set(ctx->stream, x, ctx->ghost_idx.p, ctx->ghost_zero.p, ctx->nghost);
}
int rebuild_matrix_bc(FsiCtx* ctx) {
  std::vector<int32_t> m(ctx->h_bc);
  m.insert(m.end(), ctx->h_ident.begin(), ctx->h_ident.end());
  ctx->nmbc = (int64_t)m.size();
  return upload(ctx, ctx->mbc_dofs, m);
}

}  // namespace host
}  // namespace fsi

// =========================================================================================================
extern "C" {

int fsi_set_chebyshev(FsiCtx* ctx, int32_t its_solid, double kappa_solid, int32_t its_fluid, double kappa_fluid,
                      int32_t its_schur, double kappa_schur, int32_t its_disp, double kappa_disp) {
  if (!ctx) return FSI_ERR_INVALID;
  if (its_disp > 0) ctx->cheb_its_d = its_disp;
  if (kappa_disp > 1.0) ctx->cheb_kappa_d = kappa_disp;
  if (its_solid > 0) ctx->cheb_its_s = its_solid;
  if (kappa_solid > 1.0) ctx->cheb_kappa_s = kappa_solid;
  if (its_fluid > 0) ctx->cheb_its_f = its_fluid;
  if (kappa_fluid > 1.0) ctx->cheb_kappa_f = kappa_fluid;
  if (its_schur > 0) ctx->cheb_its_p = its_schur;
  if (kappa_schur > 1.0) ctx->cheb_kappa_p = kappa_schur;
  gcr_reset(ctx);     // the recycled directions were built with another (fixed) preconditioner
  return FSI_OK;
}

int fsi_set_newton_forcing(FsiCtx* ctx, double forcing) {
  if (!ctx || !(forcing >= 0.0)) return FSI_ERR_INVALID;
  ctx->newton_forcing = forcing;
  return FSI_OK;
}

int fsi_set_linear_solver(FsiCtx* ctx, int32_t precond) {
  if (!ctx || precond < 0 || precond > 1) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  const bool changed = precond != ctx->precond;
  ctx->precond = precond;
  if (changed && ctx->have_jacobian) { gcr_reset(ctx); return refresh_preconditioner(ctx); }
  return FSI_OK;
}

const char* fsi_last_error(const FsiCtx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int64_t fsi_num_dofs(const FsiCtx* ctx) { return ctx ? ctx->ndof : 0; }
int64_t fsi_matrix_nnz(const FsiCtx* ctx) { return ctx ? ctx->nnz : 0; }

int fsi_device_memory(FsiCtx* ctx, int64_t* free_bytes, int64_t* total_bytes) {
  if (!ctx || !free_bytes || !total_bytes) return FSI_ERR_INVALID;
  size_t f = 0, t = 0;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return FSI_OK;
}

int fsi_get_tuning(const FsiCtx* ctx, FsiTuning* out) {
  if (!ctx || !out) return FSI_ERR_INVALID;
  fsi_tuning_copy_out(&ctx->tune, out);      // out->struct_size is in / out: at most that many bytes are written
  return FSI_OK;
}

int fsi_set_dirichlet(FsiCtx* ctx, int64_t n, const int64_t* dofs) {
  if (!ctx || n < 0 || (n > 0 && !dofs)) return FSI_ERR_INVALID;
  std::vector<int32_t> s(n);
  for (int64_t i = 0; i < n; ++i) {
    if (dofs[i] < 0 || dofs[i] >= ctx->ndof) { ctx->err = "fsi_set_dirichlet: dof out of range"; return FSI_ERR_INVALID; }
    s[i] = ctx->h_user2solver[dofs[i]];
  }
  ctx->nbc = n;
  ctx->h_bc = s;
  FSICHK(rebuild_matrix_bc(ctx));
  FSICHK(upload(ctx, ctx->bc_dofs, s));
  HIPCHK(ctx->bc_vals.alloc(n));
  if (n) HIPCHK(hipMemset(ctx->bc_vals.p, 0, n * sizeof(double)));
  return FSI_OK;
}

int fsi_set_dirichlet_values(FsiCtx* ctx, int64_t n, const double* values) {
  if (!ctx || n != ctx->nbc || (n > 0 && !values)) { if (ctx) ctx->err = "fsi_set_dirichlet_values: size mismatch"; return FSI_ERR_INVALID; }
  if (n) HIPCHK(hipMemcpy(ctx->bc_vals.p, values, n * sizeof(double), hipMemcpyHostToDevice));
  return FSI_OK;
}

int fsi_set_partition(FsiCtx* ctx, int64_t num_owned_cells, int64_t n_ghost, const int64_t* ghost_dofs,
                      int64_t n_identity, const int64_t* identity_dofs, int64_t n_send, const int64_t* send_dofs,
                      double* sendbuf_dev, double* recvbuf_dev, const FsiComm* comm) {
  if (!ctx) return FSI_ERR_INVALID;
  if (!comm || !comm->allreduce_sum || !comm->halo_exchange || num_owned_cells < 0 || num_owned_cells > ctx->C ||
      n_ghost < 0 || n_send < 0 || n_identity < 0 || n_identity > n_ghost || (n_ghost > 0 && (!ghost_dofs || !recvbuf_dev)) ||
      (n_identity > 0 && !identity_dofs) || (n_send > 0 && (!send_dofs || !sendbuf_dev))) {
    ctx->err = "fsi_set_partition: bad arguments";
    return FSI_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int32_t> g(n_ghost), idn(n_identity), sd(n_send);
  std::vector<uint8_t> is_ghost(ctx->ndof, 0);
  for (int64_t i = 0; i < n_ghost; ++i) {
    if (ghost_dofs[i] < 0 || ghost_dofs[i] >= ctx->ndof || is_ghost[ghost_dofs[i]]) { ctx->err = "fsi_set_partition: ghost dof out of range or repeated"; return FSI_ERR_INVALID; }
    is_ghost[ghost_dofs[i]] = 1;
    g[i] = ctx->h_user2solver[ghost_dofs[i]];
  }
  for (int64_t i = 0; i < n_identity; ++i) {
    if (identity_dofs[i] < 0 || identity_dofs[i] >= ctx->ndof || !is_ghost[identity_dofs[i]]) { ctx->err = "fsi_set_partition: identity dof is not a ghost dof"; return FSI_ERR_INVALID; }
    idn[i] = ctx->h_user2solver[identity_dofs[i]];
  }
  for (int64_t i = 0; i < n_send; ++i) {
    if (send_dofs[i] < 0 || send_dofs[i] >= ctx->ndof || is_ghost[send_dofs[i]]) { ctx->err = "fsi_set_partition: send dof out of range or not owned"; return FSI_ERR_INVALID; }
    sd[i] = ctx->h_user2solver[send_dofs[i]];
  }
  ctx->h_ident = idn;
  ctx->nghost = n_ghost;
  ctx->nident = n_identity;
  ctx->nsend = n_send;
  ctx->C_owned = num_owned_cells;
  FSICHK(upload(ctx, ctx->ghost_idx, g));
  FSICHK(upload(ctx, ctx->ident_idx, idn));
  FSICHK(upload(ctx, ctx->send_idx, sd));
  HIPCHK(ctx->ghost_zero.alloc(n_ghost));
  if (n_ghost) HIPCHK(hipMemset(ctx->ghost_zero.p, 0, n_ghost * sizeof(double)));
  FSICHK(rebuild_matrix_bc(ctx));
  ctx->sendbuf = sendbuf_dev;
  ctx->recvbuf = recvbuf_dev;
  ctx->comm = *comm;
  ctx->part = true;
  ctx->have_jacobian = false;
  gcr_reset(ctx);
  // whether the preconditioner sees the residual on an overlap is one decision for the whole job (a collective halo
  // update hangs if some ranks skip it): any rank with complete ghost rows switches it on for all
  double overlap = ctx->nident < ctx->nghost ? 1.0 : 0.0;
  if (ctx->comm.allreduce_sum(ctx->comm.user, &overlap, 1) != 0) { ctx->err = "allreduce callback failed"; return FSI_ERR_DEVICE; }
  ctx->ras = overlap > 0.0;
  return FSI_OK;
}

int fsi_rccl_unique_id(void* id128) {
  if (!id128) return FSI_ERR_INVALID;
  std::string err;
  return rccl_unique_id(id128, &err);
}

int fsi_set_rccl(FsiCtx* ctx, const void* id128, int32_t rank, int32_t world, const int64_t* send_counts, const int64_t* recv_counts) {
  if (!ctx) return FSI_ERR_INVALID;
  if (!id128) {                // back to the FsiComm callbacks of fsi_set_partition (the communicator, if any, is destroyed)
    HIPCHK(hipSetDevice(ctx->device));
    rccl_destroy(ctx);
    return FSI_OK;
  }
  if (world < 1 || rank < 0 || rank >= world || !send_counts || !recv_counts) { ctx->err = "fsi_set_rccl: bad arguments"; return FSI_ERR_INVALID; }
  return rccl_init(ctx, id128, rank, world, send_counts, recv_counts);
}

int fsi_set_pressure_facets(FsiCtx* ctx, int64_t nf, const int32_t* facet_nodes, const int32_t* plus_cell) {
  if (!ctx || nf < 0 || (nf > 0 && (!facet_nodes || !plus_cell))) return FSI_ERR_INVALID;
  std::vector<int32_t> dofs;
  std::vector<double> coef;
  const double* X = ctx->h_coords.data();
  for (int64_t f = 0; f < nf; ++f) {
    const int32_t* fn = facet_nodes + 6 * f;
    const int32_t cell = plus_cell[f];
    if (cell < 0 || cell >= ctx->C) { ctx->err = "fsi_set_pressure_facets: bad cell"; return FSI_ERR_INVALID; }
    for (int a = 0; a < 6; ++a)
      if (fn[a] < 0 || fn[a] >= ctx->N2 || (a < 3 && fn[a] >= ctx->V)) { ctx->err = "fsi_set_pressure_facets: bad node"; return FSI_ERR_INVALID; }
    const double *a = X + 3 * fn[0], *b = X + 3 * fn[1], *c = X + 3 * fn[2];
    double e1[3], e2[3], nv[3], fc[3], cc[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) { e1[i] = b[i] - a[i]; e2[i] = c[i] - a[i]; fc[i] = (a[i] + b[i] + c[i]) / 3.0; }
    nv[0] = e1[1] * e2[2] - e1[2] * e2[1];
    nv[1] = e1[2] * e2[0] - e1[0] * e2[2];
    nv[2] = e1[0] * e2[1] - e1[1] * e2[0];       // |nv| = 2 area
    for (int v = 0; v < 4; ++v)
      for (int i = 0; i < 3; ++i) cc[i] += 0.25 * X[3 * ctx->h_tet_nodes[10 * (int64_t)cell + v] + i];
    const double sgn = (nv[0] * (fc[0] - cc[0]) + nv[1] * (fc[1] - cc[1]) + nv[2] * (fc[2] - cc[2])) < 0 ? -1.0 : 1.0;
    // int N_a ds = 0 for the vertex functions, area/3 for the edge functions (P2 triangle)
    for (int e = 3; e < 6; ++e)
      for (int i = 0; i < 3; ++i) {
        dofs.push_back(6 * ctx->h_node2rank[fn[e]] + 3 + i);
        coef.push_back(sgn * 0.5 * nv[i] / 3.0);
      }
  }
  // one entry per dof (a node's facets summed here, in facet order): the device adds each target once, so the load vector
  // does not depend on the order in which atomics arrive
  {
    std::vector<int64_t> order(dofs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int64_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return dofs[a] < dofs[b]; });
    std::vector<int32_t> udofs;
    std::vector<double> ucoef;
    for (int64_t i : order) {
      if (!udofs.empty() && udofs.back() == dofs[i]) ucoef.back() += coef[i];
      else { udofs.push_back(dofs[i]); ucoef.push_back(coef[i]); }
    }
    dofs.swap(udofs);
    coef.swap(ucoef);
  }
  ctx->npf = (int64_t)dofs.size();
  FSICHK(upload(ctx, ctx->pf_dofs, dofs));
  FSICHK(upload(ctx, ctx->pf_coef, coef));
  return FSI_OK;
}

int fsi_set_interface_pressure(FsiCtx* ctx, double P) {
  if (!ctx) return FSI_ERR_INVALID;
  ctx->P = P;
  return FSI_OK;
}

int fsi_set_robin_facets(FsiCtx* ctx, int64_t nf, const int32_t* facet_nodes, const double* k_s, const double* c_s) {
  if (!ctx || nf < 0 || (nf > 0 && (!facet_nodes || !k_s || !c_s))) return FSI_ERR_INVALID;
  // reference P2 triangle mass matrix / area: (1/180) [[6,-1,-1,-4,0,0],[-1,6,-1,0,-4,0],[-1,-1,6,0,0,-4],
  //                                                  [-4,0,0,32,16,16],[0,-4,0,16,32,16],[0,0,-4,16,16,32]]
  static const double M[6][6] = {{6, -1, -1, -4, 0, 0},  {-1, 6, -1, 0, -4, 0},  {-1, -1, 6, 0, 0, -4},
                                 {-4, 0, 0, 32, 16, 16}, {0, -4, 0, 16, 32, 16}, {0, 0, -4, 16, 16, 32}};
  std::vector<int32_t> row, col;
  std::vector<double> val;
  std::vector<int64_t> pos;
  const double* X = ctx->h_coords.data();
  std::vector<int64_t> h_rowptr(ctx->ndof + 1);
  HIPCHK(hipMemcpy(h_rowptr.data(), ctx->rowptr.p, (ctx->ndof + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  for (int64_t f = 0; f < nf; ++f) {
    const int32_t* fn = facet_nodes + 6 * f;
    for (int a = 0; a < 6; ++a)
      if (fn[a] < 0 || fn[a] >= ctx->N2 || (a < 3 && fn[a] >= ctx->V)) { ctx->err = "fsi_set_robin_facets: bad node"; return FSI_ERR_INVALID; }
    const double *a = X + 3 * fn[0], *b = X + 3 * fn[1], *c = X + 3 * fn[2];
    double e1[3], e2[3];
    for (int i = 0; i < 3; ++i) { e1[i] = b[i] - a[i]; e2[i] = c[i] - a[i]; }
    const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    const double area = 0.5 * std::sqrt(nx * nx + ny * ny + nz * nz);
    for (int p = 0; p < 6; ++p)
      for (int q = 0; q < 6; ++q) {
        const double m = area * M[p][q] / 180.0;
        if (m == 0.0) continue;
        const int32_t rp = ctx->h_node2rank[fn[p]], rq = ctx->h_node2rank[fn[q]];
        const int32_t* lo = ctx->h_nadj.data() + ctx->h_nadj_ptr[rp];
        const int32_t* hi = ctx->h_nadj.data() + ctx->h_nadj_ptr[rp + 1];
        const int64_t k = std::lower_bound(lo, hi, rq) - lo;
        for (int i = 0; i < 3; ++i) {
          const int32_t r = 6 * rp + 3 + i;
          row.push_back(r); col.push_back(6 * rq + i);     val.push_back(k_s[f] * m); pos.push_back(h_rowptr[r] + 6 * k + i);
          row.push_back(r); col.push_back(6 * rq + 3 + i); val.push_back(c_s[f] * m); pos.push_back(h_rowptr[r] + 6 * k + 3 + i);
        }
      }
  }
  // sorted by (row, column) with duplicates merged: one thread per row adds its entries in that order (residual), and every
  // matrix position is added once (A_pre) - no dependence on the order of atomics
  {
    std::vector<int64_t> order(row.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int64_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return row[a] != row[b] ? row[a] < row[b] : col[a] < col[b]; });
    std::vector<int32_t> r2, c2, urow, ptr;
    std::vector<double> v2;
    std::vector<int64_t> p2;
    for (int64_t i : order) {
      if (!r2.empty() && r2.back() == row[i] && c2.back() == col[i]) { v2.back() += val[i]; continue; }
      if (r2.empty() || r2.back() != row[i]) { urow.push_back(row[i]); ptr.push_back((int32_t)r2.size()); }
      r2.push_back(row[i]); c2.push_back(col[i]); v2.push_back(val[i]); p2.push_back(pos[i]);
    }
    ptr.push_back((int32_t)r2.size());
    row.swap(r2); col.swap(c2); val.swap(v2); pos.swap(p2);
    ctx->nrobin_rows = (int64_t)urow.size();
    FSICHK(upload(ctx, ctx->rb_urow, urow));
    FSICHK(upload(ctx, ctx->rb_ptr, ptr));
  }
  ctx->nrobin = (int64_t)row.size();
  FSICHK(upload(ctx, ctx->rb_row, row));
  FSICHK(upload(ctx, ctx->rb_col, col));
  FSICHK(upload(ctx, ctx->rb_val, val));
  FSICHK(upload(ctx, ctx->rb_pos, pos));
  return FSI_OK;
}
static double* state_ptr(FsiCtx* ctx, int which) {
  switch (which) {
    case 0: return ctx->U.p;
    case 1: return ctx->U1.p;
    case 2: return ctx->b.p;
    case 3: return ctx->du.p;
    default: return nullptr;
  }
}

int fsi_get_state(FsiCtx* ctx, int which, double* out) {
  if (!ctx || !out || !state_ptr(ctx, which)) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  launch_gather(ctx->stream, ctx->tmp7.p, state_ptr(ctx, which), ctx->user2solver.p, ctx->ndof);   // tmp7[user] = x[solver]
  HIPCHK(hipMemcpyAsync(out, ctx->tmp7.p, ctx->ndof * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_get_values(FsiCtx* ctx, int which, int64_t n, const int64_t* dofs, double* out) {
  if (!ctx || !state_ptr(ctx, which) || n < 0 || (n > 0 && (!dofs || !out))) return FSI_ERR_INVALID;
  if (n == 0) return FSI_OK;
  if (n > ctx->ndof) { ctx->err = "fsi_get_values: more dofs than the problem has"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int32_t> idx((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (dofs[i] < 0 || dofs[i] >= ctx->ndof) { ctx->err = "fsi_get_values: dof out of range"; return FSI_ERR_INVALID; }
    idx[i] = ctx->h_user2solver[dofs[i]];
  }
  if (ctx->gv_idx.n < (size_t)n) HIPCHK(ctx->gv_idx.alloc((size_t)n));
  HIPCHK(hipMemcpyAsync(ctx->gv_idx.p, idx.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_gather(ctx->stream, ctx->tmp7.p, state_ptr(ctx, which), ctx->gv_idx.p, n);
  HIPCHK(hipMemcpyAsync(out, ctx->tmp7.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_set_state(FsiCtx* ctx, int which, const double* in) {
  if (!ctx || !in || !state_ptr(ctx, which)) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(ctx->tmp7.p, in, ctx->ndof * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_scatter(ctx->stream, state_ptr(ctx, which), ctx->tmp7.p, ctx->user2solver.p, ctx->ndof);  // x[solver] = in[user]
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_get_matrix(FsiCtx* ctx, int64_t* rowptr, int64_t* cols, double* vals) {
  if (!ctx || !rowptr || !cols || !vals) return FSI_ERR_INVALID;
  if (!ctx->have_jacobian) { ctx->err = "fsi_get_matrix: no Jacobian assembled"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->ndof, nnz = ctx->nnz;
  std::vector<int64_t> rp(n + 1);
  std::vector<int32_t> cs(nnz), s2u(n);
  std::vector<double> vs(nnz), sc(n);
  HIPCHK(hipMemcpy(rp.data(), ctx->rowptr.p, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cs.data(), ctx->cols.p, nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(vs.data(), ctx->A.p, nnz * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sc.data(), ctx->rowscale.p, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s2u.data(), ctx->solver2user.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  rowptr[0] = 0;
  for (int64_t u = 0; u < n; ++u) {
    const int64_t s = ctx->h_user2solver[u];
    rowptr[u + 1] = rowptr[u] + (rp[s + 1] - rp[s]);
  }
  std::vector<std::pair<int64_t, double>> rowbuf;
  for (int64_t u = 0; u < n; ++u) {
    const int64_t s = ctx->h_user2solver[u];
    rowbuf.clear();
    for (int64_t t = rp[s]; t < rp[s + 1]; ++t) rowbuf.emplace_back((int64_t)s2u[cs[t]], vs[t] / sc[s]);
    std::sort(rowbuf.begin(), rowbuf.end());
    int64_t o = rowptr[u];
    for (auto& e : rowbuf) { cols[o] = e.first; vals[o] = e.second; ++o; }
  }
  return FSI_OK;
}

int fsi_spmv(FsiCtx* ctx, const double* x, double* y) {
  if (!ctx || !x || !y) return FSI_ERR_INVALID;
  if (!ctx->have_jacobian) { ctx->err = "fsi_spmv: no Jacobian assembled"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->ndof;
  HIPCHK(hipMemcpyAsync(ctx->tmp7.p, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_scatter(ctx->stream, ctx->tmp1.p, ctx->tmp7.p, ctx->user2solver.p, n);
  FSICHK(spmv(ctx, ctx->tmp1.p, ctx->tmp2.p));                 // the kernel of the outer Krylov method
  // undo the row equilibration: y = D^-1 (D A) x
  launch_gather(ctx->stream, ctx->tmp7.p, ctx->tmp2.p, ctx->user2solver.p, n);
  std::vector<double> ys(n), sc(n);
  HIPCHK(hipMemcpyAsync(ys.data(), ctx->tmp7.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  launch_gather(ctx->stream, ctx->tmp3.p, ctx->rowscale.p, ctx->user2solver.p, n);
  HIPCHK(hipMemcpyAsync(sc.data(), ctx->tmp3.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < n; ++i) y[i] = ys[i] / sc[i];
  return FSI_OK;
}

int fsi_apply_preconditioner(FsiCtx* ctx, const double* r, double* z) {
  if (!ctx || !r || !z) return FSI_ERR_INVALID;
  if (!ctx->have_jacobian) { ctx->err = "fsi_apply_preconditioner: no Jacobian assembled"; return FSI_ERR_INVALID; }
  if (ctx->part) { ctx->err = "fsi_apply_preconditioner: single contexts only (a partitioned one applies its rank-local part inside fsi_solve)"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->tmp7.p, r, n * sizeof(double), hipMemcpyHostToDevice, st));
  launch_scatter(st, ctx->tmp1.p, ctx->tmp7.p, ctx->user2solver.p, n);
  launch_mul(st, ctx->tmp1.p, ctx->tmp1.p, ctx->rowscale.p, n);      // the solver works on D A x = D b
  FSICHK(precondition(ctx, ctx->tmp1.p, ctx->tmp2.p));
  launch_gather(st, ctx->tmp7.p, ctx->tmp2.p, ctx->user2solver.p, n);
  HIPCHK(hipMemcpyAsync(z, ctx->tmp7.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FSI_OK;
}

int fsi_probe(FsiCtx* ctx, int64_t n, const int32_t* cells, const double* bary, double* out) {
  if (!ctx || n < 0 || (n > 0 && (!cells || !bary || !out))) return FSI_ERR_INVALID;
  if (n == 0) return FSI_OK;
  for (int64_t i = 0; i < n; ++i)
    if (cells[i] < 0 || cells[i] >= ctx->C) { ctx->err = "fsi_probe: cell out of range (locate the points first)"; return FSI_ERR_INVALID; }
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<int32_t> dc;
  DevBuf<double> db, dout;
  HIPCHK(dc.alloc(n)); HIPCHK(db.alloc(4 * n)); HIPCHK(dout.alloc(7 * n));
  HIPCHK(hipMemcpyAsync(dc.p, cells, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(db.p, bary, 4 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_probe(ctx->stream, n, elem_arrays(ctx), dc.p, db.p, ctx->U.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, 7 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_flow_stats(FsiCtx* ctx, double* out) {
  if (!ctx || !out) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->cellvals.p) HIPCHK(ctx->cellvals.alloc(2 * ctx->C + 8 + 4 * STAT_PARTS));
  double* res = ctx->cellvals.p + 2 * ctx->C;
  // partitioned: the cells this rank owns (they come first); the host combines the ranks with the owned-cell counts
  const int64_t nc = ctx->part ? ctx->C_owned : ctx->C;
  if (nc <= 0) { out[0] = 0.0; out[1] = 1e300; out[2] = -1e300; out[3] = 1e300; return FSI_OK; }
  launch_cell_stats(ctx->stream, nc, elem_arrays(ctx), ctx->U.p, ctx->cellvals.p, res);
  HIPCHK(hipGetLastError());
  double h[4];
  HIPCHK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  out[0] = h[0] / (double)nc; out[1] = h[1]; out[2] = h[2]; out[3] = h[3];
  return FSI_OK;
}

int fsi_calibration_streams(FsiCtx* ctx, int64_t bytes) {
  if (!ctx || bytes <= 0) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t have = (int64_t)ctx->KZ.n * 8;
  if (bytes > have) bytes = have;
  bytes &= ~(int64_t)255;
  launch_calibration(ctx->stream, ctx->KZ.p, bytes, ctx->gcr_out.p);      // the direction store is scratch between solves
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  gcr_reset(ctx);
  return FSI_OK;
}

int fsi_stress_strain(FsiCtx* ctx, int64_t n, const int32_t* cells, double* out) {
  if (!ctx || n < 0 || (n > 0 && (!cells || !out))) return FSI_ERR_INVALID;
  if (n == 0) return FSI_OK;
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<int32_t> kinds((size_t)ctx->C);
  HIPCHK(hipMemcpy(kinds.data(), ctx->cell_kind.p, (size_t)ctx->C * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    if (cells[i] < 0 || cells[i] >= ctx->C) { ctx->err = "fsi_stress_strain: cell out of range"; return FSI_ERR_INVALID; }
    if (kinds[cells[i]] != 1) { ctx->err = "fsi_stress_strain: cell is not a solid cell"; return FSI_ERR_INVALID; }
  }
  DevBuf<int32_t> dc;
  DevBuf<double> dout;
  HIPCHK(dc.alloc((size_t)n));
  HIPCHK(dout.alloc((size_t)n * 80));
  HIPCHK(hipMemcpyAsync(dc.p, cells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_stress_strain(ctx->stream, n, elem_arrays(ctx), elem_params(ctx), ctx->U.p, dc.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * 80 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

int fsi_wall_shear_stress(FsiCtx* ctx, int64_t nf, const int32_t* facet_cells, const int32_t* facet_local, double mu,
                          double* out) {
  if (!ctx || nf < 0 || (nf > 0 && (!facet_cells || !facet_local || !out)) || !(mu > 0.0)) return FSI_ERR_INVALID;
  if (nf == 0) return FSI_OK;
  HIPCHK(hipSetDevice(ctx->device));
  // one projection per boundary cell: a cell with several exterior facets couples them through its shared vertices
  std::vector<int32_t> ucell, mask, slot((size_t)nf);
  {
    std::vector<std::pair<int32_t, int64_t>> order((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) {
      if (facet_cells[f] < 0 || facet_cells[f] >= ctx->C || facet_local[f] < 0 || facet_local[f] > 3) {
        ctx->err = "fsi_wall_shear_stress: facet cell / local index out of range";
        return FSI_ERR_INVALID;
      }
      order[f] = {facet_cells[f], f};
    }
    std::sort(order.begin(), order.end());
    for (int64_t k = 0; k < nf; ++k) {
      if (k == 0 || order[k].first != order[k - 1].first) { ucell.push_back(order[k].first); mask.push_back(0); }
      mask.back() |= 1 << facet_local[order[k].second];
      slot[order[k].second] = (int32_t)ucell.size() - 1;
    }
  }
  const int64_t nc = (int64_t)ucell.size();
  DevBuf<int32_t> dc, dm;
  DevBuf<double> dout;
  HIPCHK(dc.alloc((size_t)nc));
  HIPCHK(dm.alloc((size_t)nc));
  HIPCHK(dout.alloc((size_t)nc * 12));
  HIPCHK(hipMemcpyAsync(dc.p, ucell.data(), (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(dm.p, mask.data(), (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_wss(ctx->stream, nc, elem_arrays(ctx), ctx->U.p, dc.p, dm.p, mu, dout.p);
  HIPCHK(hipGetLastError());
  std::vector<double> h((size_t)nc * 12);
  HIPCHK(hipMemcpyAsync(h.data(), dout.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  static const int VERTS[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
  for (int64_t f = 0; f < nf; ++f)
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 3; ++i) out[(f * 3 + k) * 3 + i] = h[((size_t)slot[f] * 4 + VERTS[facet_local[f]][k]) * 3 + i];
  return FSI_OK;
}

int64_t fsi_xcd_order(int64_t n, int64_t* unit_out) {
  if (n < 0) return -1;
  const int64_t span = fsi::xcd_span(n);
  if (unit_out)
    for (int64_t L = 0; L < span; ++L) unit_out[L] = fsi::xcd_unit(L, n);
  return span;
}

int fsi_get_solver_events(const FsiCtx* ctx, int64_t out[8]) {
  if (!ctx || !out) return FSI_ERR_INVALID;
  out[0] = ctx->ev_base[0] + ctx->newton_retries;
  out[1] = ctx->ev_base[1] + ctx->kry_fp32_failures_total;
  out[2] = ctx->ev_base[2] + ctx->gcr_restarts;
  out[3] = ctx->newton_adaptive_solves; out[4] = ctx->utol_tightened; out[5] = ctx->bcr_solves;
  out[6] = out[7] = 0;
  return FSI_OK;
}

int fsi_get_timers(FsiCtx* ctx, FsiTimers* out, int reset) {
  if (!ctx || !out) return FSI_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  for (PhaseTimer* t : {&ctx->t_res, &ctx->t_jac, &ctx->t_fac, &ctx->t_spmv, &ctx->t_prec, &ctx->t_ortho, &ctx->t_flush, &ctx->t_kry}) resolve_timer(t, t->issued);
  *out = FsiTimers{ctx->t_res.ms,  ctx->t_res.calls,  ctx->t_jac.ms,   ctx->t_jac.calls,   ctx->t_fac.ms, ctx->t_fac.calls,
                   ctx->t_spmv.ms, ctx->t_spmv.calls, ctx->t_prec.ms,  ctx->t_prec.calls,  ctx->t_ortho.ms,
                   ctx->t_ortho.calls, ctx->t_kry.ms, ctx->t_kry.calls, ctx->kry_iters,
                   ctx->inner_its[0], ctx->inner_its[1], ctx->inner_its[2], ctx->inner_calls,
                   ctx->smp_ss.t.ms, ctx->smp_ss.t.calls, ctx->solid_fp32 ? 9 * ctx->sb_nblocks : (int64_t)ctx->ss_vals.n, 3 * ctx->nS,
                   ctx->smp_db.t.ms, ctx->smp_db.t.calls, (int64_t)ctx->dd_db.n / 3, ctx->N2, ctx->smp_sc.t.ms, ctx->smp_sc.t.calls,
                   (int64_t)(ctx->dd_is_scalar && ctx->sweeps_fp32) + (ctx->tiled ? 2 : 0), (int64_t)ctx->tile_ulist.n,
                   ctx->ortho_q_cols, ctx->ortho_q_launches, ctx->ortho_z_cols, ctx->ortho_z_launches,
                   (int64_t)(ctx->kry_fp32 ? 4 : 8), ctx->ldq, ctx->ldz, ctx->kry.hw, ctx->kry.cap,
                   (int64_t)ctx->s_cols.n, ctx->V, ctx->t_flush.ms, ctx->t_flush.calls, ctx->smp_sch.t.ms, ctx->smp_sch.t.calls,
                   (int64_t)((ctx->schur_fp32 && ctx->s_vals32.p) ? ((ctx->schur_tiled && ctx->sweeps_fp16 && ctx->s_rec.p) ? 0 : 4) : 8),
                   (int64_t)ctx->h_nadj.size(), (int64_t)ctx->h_padj.size(),
                   ctx->prod.products32,
                   (int64_t)((ctx->tiled && ctx->fused_sweeps ? 1 : 0) | (ctx->tiled && ctx->fused_sweeps && ctx->sweeps_fp16 ? 2 : 0) |
                             (ctx->solid_fp32 ? 4 : 0) | (ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused ? 8 : 0) |
                             (ctx->sbmg_ready ? 16 : 0) | (ctx->mg_ready ? 32 : 0) | (ctx->prod.pairs() ? 64 : 0)),
                   ctx->part_allreduces, (int64_t)ctx->ncellcol, ctx->gcr_arnoldi_steps, ctx->gcr_restarts, ctx->newton_retries,
                   (int64_t)ctx->kry_fp32_failures_total, ctx->verdicts_skipped, ctx->gcr_reorth_forced, ctx->dd_cache_hits,
                   ctx->newton_late_solves};
  if (reset) {
    for (PhaseTimer* t : {&ctx->t_res, &ctx->t_jac, &ctx->t_fac, &ctx->t_spmv, &ctx->t_prec, &ctx->t_ortho, &ctx->t_flush, &ctx->smp_sch.t, &ctx->t_kry, &ctx->smp_ss.t, &ctx->smp_db.t, &ctx->smp_sc.t}) {
      t->ms = 0.0;
      t->calls = 0;
    }
    ctx->kry_iters = 0;
    ctx->prod.products32 = 0;
    ctx->inner_its[0] = ctx->inner_its[1] = ctx->inner_its[2] = 0;
    ctx->inner_calls = 0;
    ctx->ortho_q_cols = ctx->ortho_q_launches = ctx->ortho_z_cols = ctx->ortho_z_launches = 0;
    ctx->part_allreduces = 0;
    ctx->ev_base[0] += ctx->newton_retries; ctx->ev_base[1] += ctx->kry_fp32_failures_total; ctx->ev_base[2] += ctx->gcr_restarts;   // run totals survive
    ctx->gcr_arnoldi_steps = ctx->gcr_restarts = ctx->newton_retries = ctx->kry_fp32_failures_total = 0;
    ctx->verdicts_skipped = ctx->gcr_reorth_forced = 0;
    ctx->dd_cache_hits = ctx->newton_late_solves = 0;
    ctx->sample_budget = 16;      // the sweep kernels of the next 16 preconditioner applications are sampled with events
  }
  return FSI_OK;
}

}  // extern "C"
