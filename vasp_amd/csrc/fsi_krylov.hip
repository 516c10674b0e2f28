// Krylov methods on the row-equilibrated monolithic Jacobian: right-preconditioned GCR whose directions are kept while the
// Jacobian is kept (solve_gcr: FP32 / FP64 basis, restarts from the FP64 residual, safeguards of DESIGN.md section 5), BiCGStab
// (FsiNewtonOpts.lin_solver = 1), and the callers' entry of the monolithic product (the product itself: fsi_product.hip).
// Kernels: fsi_gcr.hip, fsi_solver.hip.  What of GCR needs no device - the store's slots, the coefficient algebra, the
// policies - is in fsi_gcr_host.hpp.
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace fsi {
namespace host {

// working = true: the product inside a Krylov iteration (MonoProduct::apply decides what it runs on)
int spmv(FsiCtx* ctx, const double* x, double* y, bool working) {
  Phase ph(ctx, &ctx->t_spmv);
  if (ctx->prod.apply(ctx, x, y, working) != 0) {
    ctx->err = "spmv: d rows in pair form without the node graph";
    return FSI_ERR_INVALID;
  }
  return FSI_OK;
}


}  // namespace host
}  // namespace fsi

// ---- GCR with directions kept across solves while the matrix is unchanged ----------------------------------
// Right-preconditioned, flexible; Q = A P orthonormal.  Per iteration only Q streams through HBM (two passes: the
// coefficients and the update, fsi_gcr.hip) and the host reads two small results; P is touched once per solve.
namespace fsi {
namespace host {

void gcr_reset(FsiCtx* ctx) {
  ctx->gs_rtol = 0.0;
  ctx->f32_last_drift = -1.0;                // no verified cycle yet on this store
  ctx->f64_suspect = false;                  // the pairs that were suspected are gone
  ctx->kry.reset();
}

}  // namespace host
}  // namespace fsi

namespace {

// device -> pinned host read of `cnt` doubles; the only host waits of the Krylov loop go through here
int gcr_read(FsiCtx* ctx, const double* dptr, int cnt, double* host) {
  HIPCHK(hipMemcpyAsync(host, dptr, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}
size_t qbytes(const FsiCtx* ctx) { return ctx->kry_fp32 ? sizeof(float) : sizeof(double); }

// What the steps of one gcr_cycle share
struct Cycle {
  double* r;                   // the current residual, updated by recurrence
  double* x;
  double target;
  int* iters;
  GcrCycle cy;
  GcrStaging lay;
  double reorth = 0.0;
  double rn2 = 0.0, r_entry = 0.0, rnorm = 0.0;
  const double* src = nullptr; // what the next direction is made from
  double* qd = nullptr;        // where the update kernel leaves the exact q: a window column (FP32 basis) or the store column itself
  bool rr_pending = false;     // partitioned: the last update's local |r|^2 has not been all-reduced yet (it rides with the next pass)
  // the iteration under way
  int slot = 0, m = 0;         // the new direction's slot; columns scanned
  std::vector<double> htot;    // [m] its coefficients on the kept columns, all passes together
  double wn = 0.0, wr = 0.0, w0 = 0.0, w_first = 0.0;
  Cycle(int64_t cap, double* r_, double* x_, double target_, int* iters_) : r(r_), x(x_), target(target_), iters(iters_), cy(cap), lay{cap} {}
};

// diagnostics behind FSI_DEBUG_GCR / FSI_DEBUG_TRUERES (at the end of the file)
void dbg_partitioned_pass(FsiCtx* ctx, const Cycle& c, int pass, double hsq, int nh);
void dbg_pass_columns(FsiCtx* ctx, const double* hh, int m, int pass, double wn2);
void dbg_iteration(FsiCtx* ctx, const Cycle& c, double alpha);
void dbg_fp32_cycle(int cyc, double rec32, double target, double rnorm, double bnorm, double rtol, int iters);
int dbg_solve(FsiCtx* ctx, const double* rhs, double* x, double* r, double rtol, double bnorm, double rnorm, int iters);

// ---- one Gram-Schmidt pass: h = Q^T w, w -= Q h ---------------------------------------------------------------------------------
enum class GsReduce {
  none,    // single context: the update kernel reads the coefficients from device memory, so it is queued right behind the
           // product kernel and the host reads both results in one wait per pass
  host,    // the coefficients go through the host, which sums them over the ranks of a partitioned run, and back
  rccl     // partitioned, the library's own communicator: summed where they are, read once per pass as in a single context
};
struct GsBasis {
  const void* Q;
  bool f32;            // storage of the columns
  int cols;
  int lead;            // how many of them, from the first, hold data; the others are taken as zeros unread (GcrStore::lead)
  double* hcoef;       // device [gcr_coef_len(cols)]
  double* stage;       // pinned [gcr_coef_len(cols)]: where the host finds the coefficients and |w|^2, w.r (GcrStaging)
  int weight;          // ortho_q_cols counts a column this many times (FP64 columns counted as two FP32 ones)
};
struct GsPass {
  GsBasis basis;
  double* w;
  const double* r = nullptr;        // w'.r from the update kernel, and (reduced passes) w.r with the coefficients; nullptr: not needed
  double* out = nullptr;            // device [2]: the update kernel's |w'|^2, w'.r
  GsReduce reduce = GsReduce::none;
  bool lagged_slot = false;         // reduced passes: one more number rides with the coefficients' reduction ...
  const double* lagged = nullptr;   // ... from here (device; nullptr: zero)
  int after = 0;                    // how many of the update kernel's two results the host needs (summed over the ranks)
  bool defer = false;               // none: leave the read queued - the next pass's wait brings it (stream order: the copy sees the values before hcoef is reused)
  bool entry = false;               // the projection on entry: the caller brackets the whole pass, waits included, and its reductions are not the iterations'
};
GsBasis store_basis(FsiCtx* ctx, int m) {
  return {ctx->KQ.p, ctx->kry_fp32 != 0, m, (int)std::min<int64_t>(m, ctx->kry.lead()), ctx->hcoef.p, ctx->gcr_host, 1};
}
GsBasis window_basis(FsiCtx* ctx, int nh) {
  return {ctx->KQh.p, false, nh, nh, ctx->hcoef_hot.p, ctx->gcr_host + GcrStaging{ctx->kry.cap}.window(), 2};
}

// after[0..2): |w'|^2 and w'.r as the update kernel measured them (p.after > 0 and not deferred)
int gs_pass(FsiCtx* ctx, const GsPass& p, double* after) {
  hipStream_t st = ctx->stream;
  const GsBasis& b = p.basis;
  const int64_t n = ctx->ndof;
  const int m = b.cols;
  const int64_t lag = GcrStaging::lagged(m), upd = GcrStaging::updated(m);      // (the device coefficients have the staging area's layout)
  const int nsum = (int)lag, nred = nsum + (p.lagged_slot ? 1 : 0);             // the coefficients and their two sums; what a reduction carries
  double* hh = b.stage;
  int launches = 0;
  auto dots = [&](const double* r) { launch_gcr_dots_lead(st, b.f32, b.Q, ctx->ldq, n, m, b.lead, p.w, r, ctx->scratch.p, b.hcoef); launches += 1; };
  auto axpy = [&] { launch_gcr_axpy_lead(st, b.f32, b.Q, ctx->ldq, n, m, b.lead, b.hcoef, p.w, p.r, ctx->scratch.p, p.out); launches += 1; };
  // The phase timer brackets the kernels only, not the host's wait.
  auto timed = [&](auto&& launch) {
    if (p.entry) { launch(); return; }
    Phase ph(ctx, &ctx->t_ortho);
    launch();
  };
  double exact[2] = {0.0, 0.0};
  switch (p.reduce) {
    case GsReduce::none:
      timed([&] { dots(nullptr); axpy(); });
      HIPCHK(hipMemcpyAsync(hh, b.hcoef, (size_t)nsum * sizeof(double), hipMemcpyDeviceToHost, st));
      if (p.after) HIPCHK(hipMemcpyAsync(hh + upd, p.out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
      if (p.defer) break;
      HIPCHK(hipStreamSynchronize(st));
      if (p.after) { exact[0] = hh[upd]; exact[1] = hh[upd + 1]; }
      break;
    case GsReduce::host:
      timed([&] { dots(p.r); });
      HIPCHK(hipMemcpyAsync(hh, b.hcoef, (size_t)nsum * sizeof(double), hipMemcpyDeviceToHost, st));
      if (p.lagged) HIPCHK(hipMemcpyAsync(hh + lag, p.lagged, sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (p.lagged_slot && !p.lagged) hh[lag] = 0.0;
      if (ctx->part) {
        FSICHK(allreduce(ctx, hh, nred));
        HIPCHK(hipMemcpyAsync(b.hcoef, hh, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
      }
      if (m == 0) break;
      timed([&] { axpy(); });
      if (p.after) {
        FSICHK(gcr_read(ctx, p.out, 2, exact));
        FSICHK(allreduce(ctx, exact, p.after));
      }
      break;
    case GsReduce::rccl:
      // the library's own communicator: the reductions run on the vectors where they are (device memory, solver stream)
      // and the update kernel is queued right behind them; the host reads the reduced numbers once per pass, for its
      // bookkeeping, exactly as in a single context
      timed([&] { dots(p.r); });
      if (p.lagged) HIPCHK(hipMemcpyAsync(b.hcoef + lag, p.lagged, sizeof(double), hipMemcpyDeviceToDevice, st));
      else if (p.lagged_slot) HIPCHK(hipMemsetAsync(b.hcoef + lag, 0, sizeof(double), st));
      FSICHK(rccl_allreduce_dev(ctx, b.hcoef, nred));
      timed([&] { axpy(); });
      if (p.after) {
        FSICHK(rccl_allreduce_dev(ctx, p.out, p.after));
        HIPCHK(hipMemcpyAsync(exact, p.out, sizeof exact, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipMemcpyAsync(hh, b.hcoef, (size_t)nred * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      break;
  }
  ctx->ortho_q_cols += (int64_t)launches * m * b.weight;
  ctx->ortho_q_launches += launches;
  if (ctx->part && !p.entry) ctx->part_allreduces += p.after ? 2 : 1;
  if (after) { after[0] = exact[0]; after[1] = exact[1]; }
  return FSI_OK;
}

int gcr_flush(FsiCtx* ctx, GcrCycle& cy, double* x) {
  const int64_t n = ctx->ndof;
  const int m = (int)ctx->kry.hw, knew = cy.knew();
  if (m == 0 || !cy.pending(m)) return FSI_OK;
  Phase ph(ctx, &ctx->t_flush);
  const int kw = gcr_flush_width(knew);
  const std::vector<double> pack = cy.pack(m, kw);
  HIPCHK(hipMemcpyAsync(ctx->gcr_y.p, pack.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (knew > 0) {
    HIPCHK(hipMemcpyAsync(ctx->gcr_cn.p, pack.data() + m, (size_t)m * kw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->gcr_slots.p, cy.slots.data(), (size_t)knew * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  launch_gcr_flush(ctx->stream, ctx->KZ.p, ctx->ldz, n, m, ctx->gcr_y.p, ctx->gcr_cn.p, ctx->gcr_slots.p, knew, x);
  HIPCHK(hipStreamSynchronize(ctx->stream));       // `pack` is pageable host memory: keep it alive until the copies are done
  ctx->ortho_z_cols += m;
  ctx->ortho_z_launches += 1;
  cy.clear();
  return FSI_OK;
}

// ---- the steps of a cycle ------------------------------------------------------------------------------------------------------
// projection on the recycled space: r -= Q (Q^T r), x-coefficients y = Q^T r
int gcr_project_entry(FsiCtx* ctx, Cycle& c) {
  Phase ph(ctx, &ctx->t_ortho);
  const int m = (int)ctx->kry.hw;
  GsPass p{store_basis(ctx, m), c.r};
  p.out = ctx->gcr_out.p;
  p.reduce = GsReduce::host;
  p.after = 1;
  p.entry = true;
  double after[2];
  FSICHK(gs_pass(ctx, p, after));
  const double* hh = ctx->gcr_host;
  c.rn2 = hh[c.lay.sums(m)];
  c.r_entry = std::sqrt(std::max(c.rn2, 0.0));
  if (m > 0) {
    for (int j = 0; j < m; ++j) c.cy.y[j] = ctx->kry.born[j] >= 0 ? hh[j] : 0.0;
    c.rn2 = after[0];
  }
  c.rnorm = std::sqrt(std::max(c.rn2, 0.0));
  return FSI_OK;
}

// z = M^-1 src, w = A z
int gcr_precondition_product(FsiCtx* ctx, const Cycle& c, double* z, double* w) {
  hipStream_t st = ctx->stream;
  if (ctx->part && ctx->ras) {
    // restricted additive Schwarz: the local solve sees the residual on its overlap (complete ghost rows), zero on the
    // outermost layer; below, the owners' part of the result replaces whatever the overlap produced
    double* rin = ctx->tmp4.p;
    launch_copy(st, rin, c.src, ctx->ndof);
    FSICHK(halo_update(ctx, rin));
    if (ctx->nident) launch_bc_set(st, rin, ctx->ident_idx.p, ctx->ghost_zero.p, ctx->nident);
    FSICHK(precondition(ctx, rin, z));
  } else {
    FSICHK(precondition(ctx, c.src, z));
  }
  FSICHK(halo_update(ctx, z));      // partitioned: the preconditioner is rank-local (additive Schwarz on the ghost layer)
  FSICHK(spmv(ctx, z, w, true));
  zero_ghost(ctx, w);               // ghost rows are identity rows; residual-type vectors carry zeros there
  return FSI_OK;
}

// a free slot for the new direction; when the store is full everything is made explicit first, then the oldest
// directions of its rotating part are retired in a batch
int gcr_make_room(FsiCtx* ctx, Cycle& c) {
  hipStream_t st = ctx->stream;
  GcrStore& s = ctx->kry;
  if (s.full()) {
    FSICHK(gcr_flush(ctx, c.cy, c.x));
    for (int32_t sidx : s.retire(gcr_retire_batch(s.cap))) {
      HIPCHK(hipMemsetAsync(ctx->KQ.p + (size_t)sidx * ctx->ldq * qbytes(ctx), 0, (size_t)ctx->ldq * qbytes(ctx), st));
      HIPCHK(hipMemsetAsync(ctx->KZ.p + (size_t)sidx * ctx->ldz, 0, (size_t)ctx->ldz * sizeof(double), st));
    }
    for (int k : s.window_drop_retired())
      if (ctx->KQh.p) HIPCHK(hipMemsetAsync(ctx->KQh.p + (size_t)k * ctx->ldq, 0, (size_t)ctx->ldq * sizeof(double), st));
  }
  bool clear = false;
  c.slot = s.take(&clear);
  // the slot's old q column is zero (retired) or has never been written: a fresh slot beyond the previous high-water mark must
  // not contribute, and does not - the store tells the Gram-Schmidt kernels to take it as zeros without reading it
  // (GcrStore::lead via store_basis) until gcr_store's update kernel has written it in full
  c.m = (int)s.hw;
  return FSI_OK;
}

// the iteration under way ends before gcr_store: a fresh slot's column, which nothing has written, is zeroed as the columns
// of retired slots are, because the slot stays inside the scanned range
int gcr_abandon_slot(FsiCtx* ctx, Cycle& c) {
  const int slot = ctx->kry.abandon(c.slot);
  if (slot >= 0) HIPCHK(hipMemsetAsync(ctx->KQ.p + (size_t)slot * ctx->ldq * qbytes(ctx), 0, (size_t)ctx->ldq * qbytes(ctx), ctx->stream));
  return FSI_OK;
}

// w against the kept columns: c.htot, |w'| (c.wn) and w'.r (c.wr)
int gcr_orthogonalise(FsiCtx* ctx, Cycle& c, double* w) {
  // classical Gram-Schmidt; a second pass when the first one cancelled w by more than 1 / reorth.  With recycled
  // directions w = A M^-1 r lies mostly IN the kept space, so the usual 2x criterion fires on most iterations; the
  // orthogonality lost in one pass only matters relative to the tolerance asked for.
  // The update kernel reads the coefficients from device memory, so in a single context it is queued right behind
  // the product kernel and the host reads both results in one wait per pass (partitioned: the coefficients are
  // all-reduced by the host in between).  The phase timer brackets the kernels only, not the host's wait.
  const bool f32 = ctx->kry_fp32 != 0;
  const int m = c.m;
  const double* hh = ctx->gcr_host;
  const double* hh_hot = hh + c.lay.window();      // second staging area of the pinned buffer (nh + 2 <= 34 values)
  c.htot.assign(m, 0.0);
  c.wn = c.wr = c.w0 = c.w_first = 0.0;
  // exact (FP64) Gram-Schmidt against the window of this cycle's directions first
  const int nh = f32 ? ctx->kry.window_cols() : 0;
  if (nh > 0) {
    GsPass p{window_basis(ctx, nh), w};
    p.out = ctx->gcr_out.p;
    p.reduce = ctx->part ? GsReduce::host : GsReduce::none;
    p.defer = true;      // read with the first pass below
    FSICHK(gs_pass(ctx, p, nullptr));
  }
  bool hot_pending = nh > 0;
  // Partitioned: ONE all-reduce per pass while the basis is FP64: the m coefficients, |w|^2, w.r and - riding along - this rank's
  // part of |r|^2 as the previous iteration's update kernel left it (the exact norm of the residual this iteration
  // starts from).  What the update needs follows without a second reduction: |w'|^2 = |w|^2 - |h|^2 (the pass is
  // repeated when that cancels by more than 1 / reorth, and the repeat measures |w'|^2 directly), w'.r = w.r because
  // r is kept orthogonal to every q.  With an FP32 basis the identity is not good enough: the stored columns are
  // orthonormal to 1e-7 only, |w'|^2 comes out wrong by h^T (Q^T Q - I) h, the new column is then not a unit vector
  // and every later projection on it is off by that factor (measured: a 2-rank run lost a cycle and fell back to
  // FP64, a 1-rank run needed 184 instead of 50 iterations every other time) - so the FP32 basis pays a second,
  // two-number reduction for the exact |w'|^2 and w'.r after the update of w, as in round 2.
  static const bool rccl_host = getenv("FSI_RCCL_HOST_REDUCE") != nullptr;      // debugging aid: stage the reductions through the host
  for (int pass = 0; pass < 2; ++pass) {
    GsPass p{store_basis(ctx, m), w};
    p.r = c.r;
    p.out = ctx->part ? ctx->gcr_out.p + 2 : ctx->gcr_out.p;
    p.reduce = !ctx->part ? GsReduce::none : (ctx->rccl && !rccl_host) ? GsReduce::rccl : GsReduce::host;
    p.lagged_slot = ctx->part != 0;
    p.lagged = c.rr_pending ? ctx->gcr_out.p + 4 : nullptr;
    p.after = (!ctx->part || f32) ? 2 : 0;
    double h2[2] = {0.0, 0.0};
    FSICHK(gs_pass(ctx, p, h2));
    const double w2 = hh[c.lay.sums(m)];
    if (ctx->part) {
      if (c.rr_pending) { c.rn2 = hh[c.lay.lagged(m)]; c.rr_pending = false; }      // exact |r|^2 before this iteration's update
      double hsq = 0.0;
      for (int j = 0; j < m; ++j) hsq += hh[j] * hh[j];
      if (!f32) { h2[0] = std::max(w2 - hsq, 0.0); h2[1] = hh[c.lay.sums(m) + 1]; }
      if (ctx->debug_gcr && *c.iters < 6) dbg_partitioned_pass(ctx, c, pass, hsq, nh);
    }
    if (hot_pending) {                       // the window's coefficients (read by the wait above, or all-reduced before)
      c.w0 = std::sqrt(std::max(hh_hot[nh], 0.0));
      for (int k = 0; k < nh; ++k)
        if (ctx->kry.hot_slots[k] >= 0) c.htot[ctx->kry.hot_slots[k]] += hh_hot[k];
      hot_pending = false;
    }
    if (pass == 0 && c.w0 == 0.0) c.w0 = std::sqrt(std::max(w2, 0.0));
    if (pass == 0) c.w_first = c.w0;
    for (int j = 0; j < m; ++j) c.htot[j] += hh[j];
    if (ctx->debug_gcr) dbg_pass_columns(ctx, hh, m, pass, h2[0]);
    c.wn = std::sqrt(std::max(h2[0], 0.0));
    c.wr = h2[1];
    bool lost = false;
    if (pass == 0 && (!ctx->part || f32)) {      // (gcr_orth_lost: when |w'|^2 was measured, not derived)
      lost = gcr_orth_lost(hh, m, w2, h2[0], f32 ? ctx->orth_floor32 : ctx->orth_floor64);
      if (lost) ctx->gcr_reorth_forced += 1;
    }
    if (c.wn > c.reorth * c.w0 && !lost) break;
    c.w0 = c.wn;
  }
  return FSI_OK;
}

// the new pair goes into the store, r and the coefficients of x move; decides what the next direction is made from
int gcr_store(FsiCtx* ctx, Cycle& c, const double* z, const double* w) {
  const bool f32 = ctx->kry_fp32 != 0;
  const double alpha = c.wr / c.wn;          // q . r with q = w / wn
  // the exact q: with an FP32 basis it goes into the FP64 window (ring of 32) beside the rounded column; an FP64 column IS the
  // exact q, written once, and an Arnoldi step below reads it where it is
  if (f32) c.qd = ctx->KQh.p + (size_t)ctx->kry.window_put(c.slot) * ctx->ldq;
  else c.qd = reinterpret_cast<double*>(ctx->KQ.p) + (size_t)c.slot * ctx->ldq;
  launch_gcr_update(ctx->stream, f32, ctx->KQ.p, ctx->ldq, ctx->KZ.p, ctx->ldz, c.slot, ctx->ndof, w, z, 1.0 / c.wn, alpha, c.r,
                    f32 ? c.qd : nullptr, ctx->scratch.p, ctx->gcr_out.p + 4);
  c.src = c.r;
  // A direction that left the residual where it was (alpha^2 below 1e-3 |r|^2): A M^-1 r lies in the kept space, and as r
  // has not moved the next A M^-1 r is the same vector again - GCR proper cannot leave this point (seen on the 100 k-tet
  // mesh: |r| constant to four digits for 40 iterations until the stagnation rule ended the cycle, and again in the next
  // solve, which then lost the FP32 basis and the recycled space).  The next direction is made from the q just stored
  // instead (an Arnoldi step: the Krylov space of A M^-1 keeps growing whatever r does) until the residual moves again.
  if (alpha * alpha <= ctx->gcr_escape * c.rnorm * c.rnorm) { c.src = c.qd; ctx->gcr_arnoldi_steps += 1; }
  // coefficients of the new direction on the store:  p = (z - sum_j h_j p_j) / wn
  c.cy.add(c.slot, c.htot.data(), c.m, c.wn, alpha);
  ctx->kry.set_born(c.slot);
  *c.iters += 1;
  ctx->kry_iters += 1;
  // |r|: the recurrence value; read back (it is one host wait, shared with nothing else) because the analytic
  // |r|^2 - alpha^2 loses its digits exactly when the iteration converges fast
  double* hh = ctx->gcr_host;
  if (ctx->part) {
    // |r'|^2 = |r|^2 - alpha^2 from the exact |r|^2 this iteration started with; the exact value of |r'|^2 (this rank's
    // part is in gcr_out[4]) travels with the next pass's reduction.  Only an iteration that looks converged pays a
    // reduction of its own, to be sure.
    c.rn2 = std::max(c.rn2 - alpha * alpha, 0.0);
    c.rr_pending = true;
    if (std::sqrt(c.rn2) <= c.target || !std::isfinite(c.rn2)) {
      FSICHK(gcr_read(ctx, ctx->gcr_out.p + 4, 1, hh));
      FSICHK(allreduce(ctx, hh, 1));
      ctx->part_allreduces += 1;
      c.rn2 = hh[0];
      c.rr_pending = false;
    }
    c.rnorm = std::sqrt(std::max(c.rn2, 0.0));
  } else {
    FSICHK(gcr_read(ctx, ctx->gcr_out.p + 4, 1, hh));
    c.rnorm = std::sqrt(std::max(hh[0], 0.0));
  }
  if (ctx->debug_gcr) dbg_iteration(ctx, c, alpha);
  return FSI_OK;
}

// One cycle: reduce |r| (r holds the current residual, updated by recurrence) to `target` (absolute).  x accumulates.
int gcr_cycle(FsiCtx* ctx, double* r, double* x, double target, double rtol_floor, int max_it, int* iters, double* rnorm_out) {
  const bool f32 = ctx->kry_fp32 != 0;
  double* z = ctx->tmp2.p;
  double* w = ctx->tmp3.p;
  Cycle c(ctx->kry.cap, r, x, target, iters);
  c.reorth = gcr_reorth_threshold(f32, ctx->part != 0, rtol_floor, ctx->gcr_reorth);
  ctx->kry.clear_window();      // FP64 window: directions of this cycle only
  FSICHK(gcr_project_entry(ctx, c));
  // New directions are made from the residual (GCR).  FSI_GCR_ARNOLDI=1 makes them from the latest q instead (the same
  // Krylov space in exact arithmetic, without the cancellation of A M^-1 r_k against the previous direction after a step
  // of little progress) - measured on the 6.6 k-tet fixture: twice the iterations and stagnation near 1e-3, because the
  // FP32 sweeps of the preconditioner resolve what is large in their input, and only the residual has the components
  // that still matter as its large ones.
  c.src = r;
  double best = c.rnorm;
  int since_gain = 0;
  ctx->gcr_stagnated = false;
  ctx->gcr_stalled = false;
  while (c.rnorm > target && *iters < max_it) {
    const GcrEnd end = gcr_cycle_end(since_gain, f32, c.rnorm, target, c.r_entry, ctx->kry.full());
    if (end == GcrEnd::stagnated) { ctx->gcr_stagnated = true; break; }
    if (end == GcrEnd::stalled) { ctx->gcr_stalled = true; break; }
    FSICHK(gcr_precondition_product(ctx, c, z, w));
    FSICHK(gcr_make_room(ctx, c));
    if (const int rc = gcr_orthogonalise(ctx, c, w)) { (void)gcr_abandon_slot(ctx, c); return rc; }
    if (!(c.wn > 0.0) || !std::isfinite(c.wn)) {
      FSICHK(gcr_abandon_slot(ctx, c));
      char buf[200];
      snprintf(buf, sizeof buf, "GCR breakdown (A M^-1 r vanished or is not finite): |w'| %.3e, |w| %.3e, w.r %.3e, %d kept, iteration %d", c.wn, c.w0, c.wr, c.m, *iters);
      ctx->err = buf;
      return FSI_ERR_LINEAR;
    }
    FSICHK(gcr_store(ctx, c, z, w));
    if (!std::isfinite(c.rnorm)) { ctx->err = "GCR diverged (non-finite residual)"; return FSI_ERR_LINEAR; }
    if (c.rnorm < 0.9 * best) { best = c.rnorm; since_gain = 0; } else since_gain += 1;
    if (c.cy.knew() == GCR_FLUSH_BATCH) FSICHK(gcr_flush(ctx, c.cy, x));
  }
  FSICHK(gcr_flush(ctx, c.cy, x));
  *rnorm_out = c.rnorm;
  return FSI_OK;
}

// ---- the steps of a solve ------------------------------------------------------------------------------------------------------
struct Solve {
  const double* rhs;
  double* x;
  double* r;
  double rtol;                 // tightened when an adaptive solve (ctx->utol) leaves too much in the unscaled norm
  int max_it;
  int* iters;
  double* relres;
  double bnorm = 0.0, rnorm = 0.0, rstart = 0.0;
  int stalls = 0;
  bool near_ok = false;
};

// r = b - A x with the FP64 matrix, and its norm
int true_residual(FsiCtx* ctx, Solve& s) {
  FSICHK(halo_update(ctx, s.x));
  FSICHK(spmv(ctx, s.x, ctx->tmp3.p));
  zero_ghost(ctx, ctx->tmp3.p);
  launch_axpby(ctx->stream, s.r, 1.0, s.rhs, -1.0, ctx->tmp3.p, ctx->ndof);
  return gnorm2(ctx, s.r, &s.rnorm);
}

// FP64 basis.  The recurrence residual is only as good as the kept pairs: x is built from the directions p_k, the
// recurrence from q_k, and A p_k = q_k holds to round-off TIMES what the recursion p_k = (z_k - sum_j h_jk p_j) / |w'|
// has amplified - measured on the known-answer case driven to 1e-11: 1e-9 for the pairs of a fresh Jacobian, 5e-6 within
// 33 directions of a hard solve (every step cancelling w a hundredfold), 1e+2 a Jacobian lifetime later, with the
// recurrence reporting 1e-11 all along.  So the answer of every cycle is judged on b - A x with the FP64 matrix (one
// product, as the FP32 basis always did), the next cycle starts from that residual (iterative refinement over the
// pairs' inconsistency), and a cycle that does not halve the true residual means the kept pairs are no longer pairs:
// they are dropped.  (When the verdict is taken: gcr_verdict_due.)
int judge_fp64_cycle(FsiCtx* ctx, Solve& s, const GcrVerdictIn& v, bool* done) {
  *done = true;
  if (!gcr_verdict_due(v, ctx->kry_fp32_policy == 3, ctx->f64_suspect)) return FSI_OK;
  const double rec64 = s.rnorm;
  FSICHK(true_residual(ctx, s));
  if (std::fabs(s.rnorm - rec64) > 0.1 * s.rtol * s.bnorm) ctx->f64_suspect = true;
  if (s.rnorm <= s.rtol * s.bnorm) return FSI_OK;
  // attainable accuracy: a tolerance at round-off level (1e-11 on a system with the 1e7 penalty rows) may be met by the
  // recurrence and missed by a factor of a few by b - A x; a second verified cycle that is still within 100x is as good
  // as FP64 makes it, and Newton's own residual check judges the step
  if (s.rtol <= 1e-9 && s.rnorm <= 100.0 * s.rtol * s.bnorm && (ctx->gcr_stagnated || v.cyc >= 1)) { s.near_ok = true; return FSI_OK; }
  if (*s.iters >= s.max_it) return FSI_OK;
  if (ctx->gcr_stalled || !(s.rnorm < 0.5 * s.rstart)) {      // (stalled: the truncated recurrence of a full store made no progress)
    if (s.stalls >= 2) return FSI_OK;
    s.stalls += 1;
    ctx->gcr_restarts += 1;
    gcr_reset(ctx);                      // x keeps what the flushed directions gave it
  }
  *done = false;
  return FSI_OK;
}

// FP32 basis: with the FP32 copy of the matrix in the iterations every answer is judged on the residual of the FP64 matrix
// before it is returned (one FP64 product per cycle); without it, every answer asked for below 1e-4 - unless the verdict may
// be skipped (gcr_verdict_skippable)
int judge_fp32_cycle(FsiCtx* ctx, Solve& s, const GcrVerdictIn& v, double target, bool* done) {
  *done = true;
  const bool final_cycle = target <= s.rtol * s.bnorm * (1.0 + 1e-12);
  if (final_cycle && s.rtol >= 1e-4 && !ctx->prod.copy_ok) return FSI_OK;
  if (gcr_verdict_skippable(v, ctx->in_newton, final_cycle, ctx->f32_verdict_skip_rtol, ctx->f32_last_drift)) {
    ctx->verdicts_skipped += 1;
    return FSI_OK;
  }
  const double rec32 = s.rnorm;
  FSICHK(true_residual(ctx, s));
  ctx->f32_last_drift = std::fabs(s.rnorm - rec32) / s.bnorm;
  if (getenv("FSI_DEBUG_TRUERES")) dbg_fp32_cycle(v.cyc, rec32, target, s.rnorm, s.bnorm, s.rtol, *s.iters);
  if (s.rnorm <= s.rtol * s.bnorm) return FSI_OK;
  *done = false;
  if (s.rnorm < 0.5 * s.rstart) return FSI_OK;
  // the cycle did not bring the true residual down: FP32 storage has lost this system (a tolerance near round-off,
  // or a cancellation the FP64 window did not cover).  Drop the kept directions and finish in FP64 from here.
  if (ctx->kry_fp32_policy == 1) {
    // FSI_KRYLOV_FP32=1 sized the basis store for 4-byte columns: there is no FP64 store to fall back to, and
    // addressing it with 8-byte columns would run past the allocation.  The policy was forced, so say so.
    char buf[200];
    snprintf(buf, sizeof buf, "GCR: the FP32 Krylov basis forced by FSI_KRYLOV_FP32=1 cannot reach rtol %.1e on this system "
             "(true residual %.3e of |b| after a cycle); use the default policy", s.rtol, s.rnorm / s.bnorm);
    ctx->err = buf;
    *s.relres = s.rnorm / s.bnorm;
    return FSI_ERR_LINEAR;
  }
  // (Tried in round 3: dropping the kept pairs once and staying FP32 before giving FP32 up - on a full store late in a
  // Jacobian's life the solves that follow then need 200+ iterations each and the 100-step run loses a third: the FP64
  // basis for the rest of the lifetime is the cheaper answer.)
  gcr_reset(ctx);
  ctx->kry_fp32 = 0;
  if (ctx->kry_fp32_policy == 2) {      // FP64 for the rest of this Jacobian's life; re-armed at the next refresh (twice at most)
    ctx->kry_fp32_policy = 3;
    ctx->kry_fp32_failures += 1;
    ctx->kry_fp32_failures_total += 1;
  }
  return FSI_OK;
}

// cycles at one tolerance, each judged, until an answer stands or the iterations are spent
int run_cycles(FsiCtx* ctx, Solve& s) {
  for (int cyc = 0; cyc < 8 && *s.iters < s.max_it; ++cyc) {
    // FP32 storage of Q: the residual recurrence of one cycle is good to about 1e-6 of the residual the cycle started from;
    // a tighter request is met by restarting the cycle from the true residual b - A x (iterative refinement).
    const bool f32 = ctx->kry_fp32 != 0;
    // (measured on the bench workload, round 3: at a recurrence residual of 6e-6 |b| the true one differs in the third digit,
    // at 1e-2 not in the fourth; the first solve on a fresh FP32 store is the exception - 6e-5 against 4e-4 - and the
    // verdict below catches it.  A cycle may therefore run down to 1e-6 of its start; round 2's 1e-5 cost every first solve
    // of a time step - tolerances of 3e-6 .. 9e-6 - a second cycle: one more FP64 product and two passes over Q.)
    const double target = f32 ? std::max(s.rtol * s.bnorm, ctx->f32_cycle_floor * s.rstart) : s.rtol * s.bnorm;
    const int its0 = *s.iters;
    FSICHK(gcr_cycle(ctx, s.r, s.x, target, ctx->gs_rtol, s.max_it, s.iters, &s.rnorm));
    const GcrVerdictIn v{s.rtol, s.rnorm, s.bnorm, cyc, *s.iters - its0, ctx->gcr_stagnated, ctx->gcr_stalled, ctx->kry.full()};
    bool done = false;
    FSICHK(f32 ? judge_fp32_cycle(ctx, s, v, target, &done) : judge_fp64_cycle(ctx, s, v, &done));
    if (done) break;
    s.rstart = s.rnorm;
  }
  return FSI_OK;
}

}  // namespace

namespace fsi {
namespace host {

int solve_gcr(FsiCtx* ctx, const double* rhs, double* x, double rtol_in, int max_it, int* iters, double* relres) {
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  Solve s{rhs, x, ctx->tmp1.p, rtol_in, max_it, iters, relres};
  launch_copy(st, s.r, rhs, n);
  launch_fill(st, x, n, 0.0);
  FSICHK(gnorm2(ctx, s.r, &s.bnorm));
  *iters = 0;
  if (s.bnorm == 0.0) { *relres = 0.0; return FSI_OK; }
  if (!std::isfinite(s.bnorm)) { ctx->err = "non-finite right-hand side"; return FSI_ERR_LINEAR; }
  // storage of Q for this Jacobian's lifetime, decided by the first solve after the refresh (gcr_basis_fp32)
  if (ctx->kry.hw == 0 && ctx->kry_fp32_policy == 3) ctx->kry_fp32 = 0;
  if (ctx->kry.hw == 0 && ctx->kry_fp32_policy == 2) ctx->kry_fp32 = gcr_basis_fp32(ctx->tol_hint, s.rtol, ctx->tune.krylov_fp32_floor);
  s.rtol = gcr_adaptive_start(s.rtol, ctx->utol, ctx->utol_ratio, ctx->utol_rtol_floor);
  // the kept directions serve every later solve with this matrix, so the tightest tolerance asked for since the refresh
  // decides the re-orthogonalisation criterion, not this solve's
  ctx->gs_rtol = ctx->gs_rtol > 0.0 ? std::min(ctx->gs_rtol, s.rtol) : s.rtol;
  s.rstart = s.rnorm = s.bnorm;
  for (int tighten = 0; tighten < 8; ++tighten) {
    FSICHK(run_cycles(ctx, s));
    // adaptive Newton solves: the unscaled residual D_r^-1 r against utol |b| (r: the residual the cycles ended on)
    if (!(ctx->utol > 0.0) || !(s.rnorm <= s.rtol * s.bnorm) || s.rtol <= ctx->utol_rtol_floor * (1.0 + 1e-12) || *iters >= max_it) break;
    double ru = 0.0;
    launch_div(st, ctx->tmp3.p, s.r, ctx->rowscale.p, n);
    FSICHK(gnorm2(ctx, ctx->tmp3.p, &ru));
    if (s.rnorm > 0.0 && ctx->b_unscaled > 0.0) ctx->utol_ratio = (ru / ctx->b_unscaled) / (s.rnorm / s.bnorm);
    if (!(ru > ctx->utol * ctx->b_unscaled)) break;
    s.rtol = gcr_adaptive_tighten(s.rtol, ctx->utol, ctx->b_unscaled, ru, ctx->utol_rtol_floor);
    ctx->utol_tightened += 1;
    s.rstart = s.rnorm;
  }
  *relres = s.rnorm / s.bnorm;
  if (getenv("FSI_DEBUG_TRUERES")) FSICHK(dbg_solve(ctx, rhs, x, s.r, s.rtol, s.bnorm, s.rnorm, *iters));
  // stagnation within a factor 100 of a tolerance below 1e-9 (after the restarts above): the answer is as accurate as FP64 makes it on this system, and
  // the caller (Newton's own residual check) judges the step; reported through relres
  if ((s.near_ok || ctx->gcr_stagnated) && s.rtol <= 1e-9 && s.rnorm <= 100.0 * s.rtol * s.bnorm) return FSI_OK;
  if (!(s.rnorm <= s.rtol * s.bnorm)) {
    char buf[160];
    snprintf(buf, sizeof buf, "GCR: no convergence in %d iterations (relres %.3e, tol %.1e)", *iters, *relres, s.rtol);
    ctx->err = buf;
    return FSI_ERR_LINEAR;
  }
  return FSI_OK;
}

// ---- BiCGStab, right-preconditioned ---------------------------------------------------------------------------
int solve_bicgstab(FsiCtx* ctx, const double* rhs, double* x, double rtol, int max_it, int* iters, double* relres) {
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  double *r = ctx->tmp1.p, *r0 = ctx->tmp2.p, *p = ctx->tmp3.p, *v = ctx->tmp4.p, *s = ctx->tmp5.p, *t = ctx->tmp6.p;
  double *ph = ctx->bs.p;   // preconditioned vector (bs is free once rhs was copied)
  launch_copy(st, r, rhs, n);
  launch_copy(st, r0, rhs, n);
  launch_fill(st, x, n, 0.0);
  launch_fill(st, p, n, 0.0);
  launch_fill(st, v, n, 0.0);
  double bnorm = 0.0, rnorm = 0.0;
  FSICHK(norm2(ctx, r, &bnorm));
  *iters = 0;
  if (bnorm == 0.0) { *relres = 0.0; return FSI_OK; }
  rnorm = bnorm;
  double rho = 1.0, alpha = 1.0, omega = 1.0;
  while (rnorm > rtol * bnorm && *iters < max_it) {
    double rho1 = 0.0;
    FSICHK(dot(ctx, r0, r, &rho1));
    if (rho1 == 0.0 || !std::isfinite(rho1)) { ctx->err = "BiCGStab breakdown (rho = 0)"; return FSI_ERR_LINEAR; }
    const double beta = (rho1 / rho) * (alpha / omega);
    launch_axpy(st, p, -omega, v, n);             // p = r + beta (p - omega v)
    launch_axpby(st, p, 1.0, r, beta, p, n);
    FSICHK(precondition(ctx, p, ph));
    FSICHK(spmv(ctx, ph, v));
    double r0v = 0.0;
    FSICHK(dot(ctx, r0, v, &r0v));
    if (r0v == 0.0 || !std::isfinite(r0v)) { ctx->err = "BiCGStab breakdown (r0.v = 0)"; return FSI_ERR_LINEAR; }
    alpha = rho1 / r0v;
    launch_axpby(st, s, 1.0, r, -alpha, v, n);
    launch_axpy(st, x, alpha, ph, n);
    FSICHK(precondition(ctx, s, ph));
    FSICHK(spmv(ctx, ph, t));
    double ts = 0.0, tt = 0.0;
    FSICHK(dot(ctx, t, s, &ts));
    FSICHK(dot(ctx, t, t, &tt));
    omega = tt > 0.0 ? ts / tt : 0.0;
    launch_axpy(st, x, omega, ph, n);
    launch_axpby(st, r, 1.0, s, -omega, t, n);
    FSICHK(norm2(ctx, r, &rnorm));
    rho = rho1;
    *iters += 1;
    ctx->kry_iters += 1;
    if (omega == 0.0 && rnorm > rtol * bnorm) { ctx->err = "BiCGStab breakdown (omega = 0)"; return FSI_ERR_LINEAR; }
    if (!std::isfinite(rnorm)) { ctx->err = "BiCGStab diverged"; return FSI_ERR_LINEAR; }
  }
  *relres = rnorm / bnorm;
  // stagnation within a factor 10 of a tolerance below 1e-9: the answer is as accurate as FP64 makes it on this system, and
  // the caller (Newton's own residual check) judges the step; reported through relres
  // (gcr_stagnated is set by gcr_cycle alone: BiCGStab never sets or clears it, so what is read here is how the last GCR
  // cycle of this context ended - false in a context that has only ever run BiCGStab)
  if (ctx->gcr_stagnated && rtol <= 1e-9 && rnorm <= 10.0 * rtol * bnorm) return FSI_OK;
  if (!(rnorm <= rtol * bnorm)) {
    char buf[160];
    snprintf(buf, sizeof buf, "BiCGStab: no convergence in %d iterations (relres %.3e, tol %.1e)", *iters, *relres, rtol);
    ctx->err = buf;
    return FSI_ERR_LINEAR;
  }
  return FSI_OK;
}

}  // namespace host
}  // namespace fsi

// ---- diagnostics of the recycled GCR: FSI_DEBUG_GCR (ctx->debug_gcr), FSI_DEBUG_GCR_ALL, FSI_DEBUG_TRUERES ---------------------
namespace {

void dbg_partitioned_pass(FsiCtx* ctx, const Cycle& c, int pass, double hsq, int nh) {
  const int m = c.m;
  const double* hh = ctx->gcr_host;
  const double* hh_hot = hh + c.lay.window();
  fprintf(stderr, "[gcr]   partitioned pass %d: |w|^2 %.6e |h|^2 %.6e w.r %.6e lagged |r|^2 %.6e window: nh %d |w|^2 %.6e\n", pass, hh[m], hsq,
          hh[m + 1], hh[m + 2], nh, nh > 0 ? hh_hot[nh] : 0.0);
}

// how large the coefficients of a pass are, column by column; wn2: |w'|^2 after it
void dbg_pass_columns(FsiCtx* ctx, const double* hh, int m, int pass, double wn2) {
  const double wref = std::sqrt(std::max(hh[m], 0.0));
  for (int j = 0; j < m; ++j) {
    const double a = std::fabs(hh[j]);
    ctx->dbg_cols += 1;
    if (a > 1e-6 * wref) ctx->dbg_sig6 += 1;
    if (a > 1e-9 * wref) ctx->dbg_sig9 += 1;
    if (a > 1e-12 * wref) ctx->dbg_sig12 += 1;
  }
  if (pass != 0 || !(wn2 > 0.0)) return;
  // how many columns could have been left out of this pass with their part of w staying below 1 % of |w'| (1e-4 of |w'|^2)?
  std::vector<double> a2(m);
  for (int j = 0; j < m; ++j) a2[j] = hh[j] * hh[j];
  std::sort(a2.begin(), a2.end());
  double acc = 0.0; int drop = 0;
  for (int j = 0; j < m; ++j) { if (acc + a2[j] > 1e-4 * wn2) break; acc += a2[j]; drop += 1; }
  ctx->dbg_droppable += drop; ctx->dbg_drop_cols += m;
}

void dbg_iteration(FsiCtx* ctx, const Cycle& c, double alpha) {
  const int iters = *c.iters;
  if (getenv("FSI_DEBUG_GCR_ALL"))
    fprintf(stderr, "[gcr]     it %d: |w'|/|w| %.2e alpha/|r| %.2e |r| %.4e%s\n", iters, c.wn / std::max(c.w_first, 1e-300), alpha / std::max(c.rnorm, 1e-300), c.rnorm, c.src == c.r ? "" : " (next from q)");
  if (iters % 10 != 0) return;
  fprintf(stderr, "[gcr] it %d |r| %.3e target %.3e m %d  |h_j| > 1e-6/1e-9/1e-12 |w|: %.2f %.2f %.2f of the columns\n", iters, c.rnorm, c.target, c.m,
          (double)ctx->dbg_sig6 / std::max<int64_t>(1, ctx->dbg_cols), (double)ctx->dbg_sig9 / std::max<int64_t>(1, ctx->dbg_cols),
          (double)ctx->dbg_sig12 / std::max<int64_t>(1, ctx->dbg_cols));
  fprintf(stderr, "[gcr]   columns whose coefficients together stay below 1 %% of |w'|: %.3f of the kept ones\n", (double)ctx->dbg_droppable / std::max<int64_t>(1, ctx->dbg_drop_cols));
  fflush(stderr);
}

void dbg_fp32_cycle(int cyc, double rec32, double target, double rnorm, double bnorm, double rtol, int iters) {
  fprintf(stderr, "[gcr]   fp32 cycle %d: recurrence |r|/|b| %.3e (target %.3e), true %.3e, rtol %.1e, its %d\n", cyc, rec32 / bnorm, target / bnorm, rnorm / bnorm, rtol, iters);
}

// the answer's true residual beside the recurrence's `rnorm` (r is overwritten), and for an FP64 basis the state of the kept pairs
int dbg_solve(FsiCtx* ctx, const double* rhs, double* x, double* r, double rtol, double bnorm, double rnorm, int iters) {
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  const GcrStore& kry = ctx->kry;
  Solve s{rhs, x, r, rtol, 0, nullptr, nullptr};
  FSICHK(true_residual(ctx, s));
  fprintf(stderr, "[gcr] solve: %d its, recurrence |r|/|b| %.3e, true %.3e, kept %lld (hw %lld), restarts %lld, basis fp%d policy %d, rtol %.1e gs_rtol %.1e |b| %.3e\n", iters, rnorm / bnorm, s.rnorm / bnorm,
          (long long)kry.kept(), (long long)kry.hw, (long long)ctx->gcr_restarts, ctx->kry_fp32 ? 32 : 64, ctx->kry_fp32_policy, rtol, ctx->gs_rtol, bnorm);
  if (ctx->kry_fp32 || kry.hw == 0) return FSI_OK;
  // A p_k = q_k for the kept pairs?
  double worst = 0.0; int64_t wk = -1; double qn_w = 0.0;
  for (int64_t k = 0; k < kry.hw; ++k) {
    if (kry.born[k] < 0) continue;
    FSICHK(spmv(ctx, ctx->KZ.p + (size_t)k * ctx->ldz, ctx->tmp3.p));
    const double* qk = reinterpret_cast<const double*>(ctx->KQ.p) + (size_t)k * ctx->ldq;
    launch_axpby(st, ctx->tmp3.p, 1.0, ctx->tmp3.p, -1.0, qk, n);
    double e = 0.0, qn = 0.0;
    FSICHK(dot_n(ctx, ctx->tmp3.p, ctx->tmp3.p, n, &e));
    FSICHK(dot_n(ctx, qk, qk, n, &qn));
    const double rel = std::sqrt(e / std::max(qn, 1e-300));
    if (rel > worst) { worst = rel; wk = k; qn_w = qn; }
    if (rel > 1e-9) fprintf(stderr, "[gcr]     slot %lld born %lld: |A p - q|/|q| %.3e |q| %.6f\n", (long long)k, (long long)kry.born[k], rel, std::sqrt(qn));
  }
  fprintf(stderr, "[gcr]   worst pair: slot %lld |A p - q|/|q| %.3e (|q| %.6f)\n", (long long)wk, worst, std::sqrt(qn_w));
  // orthonormality of the kept columns: rows of Q^T Q for the last few slots
  const int mm = (int)kry.hw;
  double worst_o = 0.0; int wi = -1, wj = -1;
  for (int j = std::max(0, mm - 6); j < mm; ++j) {
    if (kry.born[j] < 0) continue;
    const double* qj = reinterpret_cast<const double*>(ctx->KQ.p) + (size_t)j * ctx->ldq;
    launch_gcr_dots(st, false, ctx->KQ.p, ctx->ldq, n, mm, qj, nullptr, ctx->scratch.p, ctx->hcoef.p);
    FSICHK(gcr_read(ctx, ctx->hcoef.p, mm + 2, ctx->gcr_host));
    for (int i = 0; i < mm; ++i) {
      if (kry.born[i] < 0) continue;
      const double dev = std::fabs(ctx->gcr_host[i] - (i == j ? 1.0 : 0.0));
      if (dev > worst_o) { worst_o = dev; wi = i; wj = j; }
    }
  }
  fprintf(stderr, "[gcr]   orthonormality of the last columns: max |q_i . q_j - delta| = %.3e (i %d, j %d)\n", worst_o, wi, wj);
  return FSI_OK;
}

}  // namespace
