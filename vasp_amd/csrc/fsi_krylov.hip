// Krylov methods on the row-equilibrated monolithic Jacobian: right-preconditioned GCR whose directions are kept while the
// Jacobian is kept (solve_gcr: FP32 / FP64 basis, restarts from the FP64 residual, safeguards of DESIGN.md section 5), BiCGStab
// (FsiNewtonOpts.lin_solver = 1), and the monolithic product.  Kernels: fsi_gcr.hip, fsi_solver.hip.
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace fsi {
namespace host {

// working = true: the product inside a Krylov iteration, which may run on the FP32 copy of the matrix while the basis of this
// Jacobian's lifetime is kept in FP32 (see solve_gcr); every other product (true residuals, the other solvers) is FP64
int spmv(FsiCtx* ctx, const double* x, double* y, bool working) {
  Phase ph(ctx, &ctx->t_spmv);
  const PRowGraph g{ctx->vrank.p, ctx->nadj_ptr.p, ctx->nadj.p};
  if (working && ctx->op32_ok && ctx->kry_fp32) {
    if (launch_spmv_node6p(ctx->stream, ctx->N2, ctx->V, ctx->a32_ptr.p, ctx->a32_cols.p, ctx->A32.p, ctx->rowptr.p, ctx->cols.p,
                           ctx->a32_ptail - ctx->a32_tail_src, g, x, y, ctx->drows_ok ? ctx->Ad32.p : nullptr) != 0) {
      ctx->err = "spmv: d rows in pair form without the node graph";
      return FSI_ERR_INVALID;
    }
    ctx->op32_products += 1;
    if (ctx->drows_ok) ctx->drows_products += 1;
    return FSI_OK;
  }
  // (drows_ok: the d rows from their pair form - six values per node pair, checked at the refresh - instead of 18 + pressure columns)
  if (launch_spmv_node6(ctx->stream, ctx->N2, ctx->V, ctx->rowptr.p, ctx->cols.p, ctx->A.p, g, x, y, ctx->drows_ok ? ctx->Ad64.p : nullptr) != 0) {
    ctx->err = "spmv: d rows in pair form without the node graph";
    return FSI_ERR_INVALID;
  }
  if (ctx->drows_ok) ctx->drows_products += 1;
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
  std::fill(ctx->hot_slots.begin(), ctx->hot_slots.end(), -1);
  ctx->hot_next = 0;
  ctx->kry_m = 0;
  ctx->kry_hw = 0;
  ctx->kry_free.clear();
  std::fill(ctx->kry_born.begin(), ctx->kry_born.end(), (int64_t)-1);
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

// One solve cycle's bookkeeping: the directions made since the last flush are p_k = sum_j cn[k][j] Z_j (Z_j explicit
// for older slots, the raw preconditioned vector for the new ones) and x = x_flushed + sum_j y[j] Z_j.
struct GcrCycle {
  std::vector<double> y;                 // [cap]
  std::vector<std::vector<double>> cn;   // knew columns of length cap
  std::vector<int32_t> slots;            // their slots
};

// retire the oldest directions of the rotating part of the store (everything explicit: call after a flush)
int gcr_retire(FsiCtx* ctx, int batch) {
  const int64_t cap = ctx->kry_cap;
  const int64_t ring = std::min<int64_t>(64, cap / 2);
  const int64_t protect = cap - ring;          // the first `protect` directions of this Jacobian stay: they resolved the hardest modes
  std::vector<std::pair<int64_t, int32_t>> cand;
  for (int64_t sidx = 0; sidx < ctx->kry_hw; ++sidx)
    if (ctx->kry_born[sidx] >= protect) cand.emplace_back(ctx->kry_born[sidx], (int32_t)sidx);
  std::sort(cand.begin(), cand.end());
  for (int k = 0; k < batch && k < (int)cand.size(); ++k) {
    const int32_t sidx = cand[k].second;
    HIPCHK(hipMemsetAsync(ctx->KQ.p + (size_t)sidx * ctx->ldq * qbytes(ctx), 0, (size_t)ctx->ldq * qbytes(ctx), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->KZ.p + (size_t)sidx * ctx->ldz, 0, (size_t)ctx->ldz * sizeof(double), ctx->stream));
    ctx->kry_born[sidx] = -1;
    ctx->kry_free.push_back(sidx);
  }
  return FSI_OK;
}

int gcr_flush(FsiCtx* ctx, GcrCycle& cy, double* x) {
  const int64_t n = ctx->ndof;
  const int m = (int)ctx->kry_hw, knew = (int)cy.slots.size();
  if (m == 0) return FSI_OK;
  bool any = knew > 0;
  for (int j = 0; j < m && !any; ++j) any = cy.y[j] != 0.0;
  if (!any) return FSI_OK;
  Phase ph(ctx, &ctx->t_flush);
  const int kw = gcr_flush_width(knew);
  std::vector<double> pack((size_t)m * (kw + 1), 0.0);
  std::copy(cy.y.begin(), cy.y.begin() + m, pack.begin());
  for (int k = 0; k < knew; ++k) std::copy(cy.cn[k].begin(), cy.cn[k].begin() + m, pack.begin() + (size_t)m * (k + 1));
  HIPCHK(hipMemcpyAsync(ctx->gcr_y.p, pack.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (knew > 0) {
    HIPCHK(hipMemcpyAsync(ctx->gcr_cn.p, pack.data() + m, (size_t)m * kw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->gcr_slots.p, cy.slots.data(), (size_t)knew * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  launch_gcr_flush(ctx->stream, ctx->KZ.p, ctx->ldz, n, m, ctx->gcr_y.p, ctx->gcr_cn.p, ctx->gcr_slots.p, knew, x);
  HIPCHK(hipStreamSynchronize(ctx->stream));       // `pack` is pageable host memory: keep it alive until the copies are done
  ctx->ortho_z_cols += m;
  ctx->ortho_z_launches += 1;
  std::fill(cy.y.begin(), cy.y.end(), 0.0);
  cy.cn.clear();
  cy.slots.clear();
  return FSI_OK;
}

// One cycle: reduce |r| (r holds the current residual, updated by recurrence) to `target` (absolute).  x accumulates.
int gcr_cycle(FsiCtx* ctx, double* r, double* x, double target, double rtol_floor, int max_it, int* iters, double* rnorm_out) {
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  const bool f32 = ctx->kry_fp32 != 0;
  double* z = ctx->tmp2.p;
  double* w = ctx->tmp3.p;
  double* hh = ctx->gcr_host;
  const int64_t cap = ctx->kry_cap;
  const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(32, cap / 4));
  GcrCycle cy;
  cy.y.assign(cap, 0.0);
  // FP32 storage: a cycle never has to reach below 1e-5 of its start, and the restart from the true residual absorbs
  // what a single pass leaves behind, so only a cancellation beyond 100x asks for the second pass
  double reorth = ctx->kry_fp32 ? 0.01 : std::min(0.5, std::max(0.01, 1.0 / (rtol_floor * 9e10)));
  if (ctx->part && !ctx->kry_fp32) reorth = std::max(reorth, 0.1);      // partitioned FP64 basis: |w'|^2 is not measured in the first pass (see below)
  if (ctx->gcr_reorth > 0.0) reorth = ctx->gcr_reorth;
  std::fill(ctx->hot_slots.begin(), ctx->hot_slots.end(), -1);      // FP64 window: directions of this cycle only
  ctx->hot_next = 0;
  double rn2 = 0.0, r_entry = 0.0;
  {   // projection on the recycled space: r -= Q (Q^T r), x-coefficients y = Q^T r
    Phase ph(ctx, &ctx->t_ortho);
    const int m = (int)ctx->kry_hw;
    launch_gcr_dots(st, f32, ctx->KQ.p, ctx->ldq, n, m, r, nullptr, ctx->scratch.p, ctx->hcoef.p);
    FSICHK(gcr_read(ctx, ctx->hcoef.p, m + 2, hh));
    ctx->ortho_q_cols += m; ctx->ortho_q_launches += 1;
    if (ctx->part) {
      FSICHK(allreduce(ctx, hh, m + 2));
      HIPCHK(hipMemcpyAsync(ctx->hcoef.p, hh, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    }
    rn2 = hh[m];
    r_entry = std::sqrt(std::max(rn2, 0.0));
    if (m > 0) {
      for (int j = 0; j < m; ++j) cy.y[j] = ctx->kry_born[j] >= 0 ? hh[j] : 0.0;
      launch_gcr_axpy(st, f32, ctx->KQ.p, ctx->ldq, n, m, ctx->hcoef.p, r, nullptr, ctx->scratch.p, ctx->gcr_out.p);
      FSICHK(gcr_read(ctx, ctx->gcr_out.p, 2, hh));
      ctx->ortho_q_cols += m; ctx->ortho_q_launches += 1;
      FSICHK(allreduce(ctx, hh, 1));
      rn2 = hh[0];
    }
  }
  double rnorm = std::sqrt(std::max(rn2, 0.0));
  // New directions are made from the residual (GCR).  FSI_GCR_ARNOLDI=1 makes them from the latest q instead (the same
  // Krylov space in exact arithmetic, without the cancellation of A M^-1 r_k against the previous direction after a step
  // of little progress) - measured on the 6.6 k-tet fixture: twice the iterations and stagnation near 1e-3, because the
  // FP32 sweeps of the preconditioner resolve what is large in their input, and only the residual has the components
  // that still matter as its large ones.
  double* qd = ctx->tmp5.p;
  const double* src = r;
  // attainable accuracy: near round-off (a tolerance of 1e-11 on a system with the 1e7 penalty) the recurrence can hover just
  // above the target for thousands of iterations; 40 iterations without a 10 % gain within a factor 100 of the target (FP32
  // basis: anywhere - the restart from the true residual is harmless) end the cycle and solve_gcr decides
  double best = rnorm;
  int since_gain = 0;
  ctx->gcr_stagnated = false;
  ctx->gcr_stalled = false;
  bool rr_pending = false;     // partitioned: the last update's local |r|^2 has not been all-reduced yet (it rides with the next pass)
  while (rnorm > target && *iters < max_it) {
    if (since_gain >= 40 && (f32 || rnorm <= 100.0 * target)) { ctx->gcr_stagnated = true; break; }
    // FP32 basis, four decades below the residual the cycle was entered with and six iterations without a 10 % gain: this is
    // the floor of the FP32 columns, not a plateau - the new q are orthogonal to the kept ones to 1e-7 times the cancellation,
    // r has collected that much of span(Q), and directions made orthogonal to Q cannot remove it.  Ending the cycle costs the
    // verdict's product and a projection, which removes it at once (48 k-tet mesh: |r| crawled from 6.05e-8 to 6.01e-8 in 37
    // iterations, and the projection that followed took it to a third of the target without a single new direction).
    if (f32 && since_gain >= 6 && rnorm <= 1e-4 * r_entry) { ctx->gcr_stagnated = true; break; }
    // Far from the target, the store full (the oldest directions kept, a ring of 64 rotating) and no 10 % gain in two turns
    // of the ring: the TRUNCATED recurrence is stuck where the full one would sit out the plateau - seen late in a Jacobian's
    // life on the known-answer case driven to round-off, |r| flat to four digits for 3 700 iterations.  solve_gcr drops the
    // kept directions and restarts from the true residual with room for a full recurrence again.  (Not applied while the
    // store still grows: plateaus of 100+ iterations are normal on these systems, and a restart inside one loses the space
    // that is about to end it.)
    if (since_gain >= 128 && ctx->kry_hw == cap && ctx->kry_free.empty()) { ctx->gcr_stalled = true; break; }
    if (ctx->part && ctx->ras) {
      // restricted additive Schwarz: the local solve sees the residual on its overlap (complete ghost rows), zero on the
      // outermost layer; below, the owners' part of the result replaces whatever the overlap produced
      double* rin = ctx->tmp4.p;
      launch_copy(st, rin, src, n);
      FSICHK(halo_update(ctx, rin));
      if (ctx->nident) launch_bc_set(st, rin, ctx->ident_idx.p, ctx->ghost_zero.p, ctx->nident);
      FSICHK(precondition(ctx, rin, z));
    } else {
      FSICHK(precondition(ctx, src, z));
    }
    FSICHK(halo_update(ctx, z));      // partitioned: the preconditioner is rank-local (additive Schwarz on the ghost layer)
    FSICHK(spmv(ctx, z, w, true));
    zero_ghost(ctx, w);               // ghost rows are identity rows; residual-type vectors carry zeros there
    // a free slot for the new direction; when the store is full everything is made explicit first, then the oldest
    // directions of its rotating part are retired in a batch
    if (ctx->kry_free.empty() && ctx->kry_hw == cap) {
      FSICHK(gcr_flush(ctx, cy, x));
      FSICHK(gcr_retire(ctx, batch));
      for (int k = 0; k < 32; ++k)
        if (ctx->hot_slots[k] >= 0 && ctx->kry_born[ctx->hot_slots[k]] < 0) {      // a retired direction leaves the window too
          ctx->hot_slots[k] = -1;
          if (ctx->KQh.p) HIPCHK(hipMemsetAsync(ctx->KQh.p + (size_t)k * ctx->ldq, 0, (size_t)ctx->ldq * sizeof(double), st));
        }
    }
    int slot;
    if (!ctx->kry_free.empty()) { slot = ctx->kry_free.back(); ctx->kry_free.pop_back(); }
    else { slot = (int)ctx->kry_hw; ctx->kry_hw += 1; }
    // the slot's old q column is zero (retired) or about to be scanned as garbage: a fresh slot beyond the previous
    // high-water mark must not contribute, so it is cleared once here
    if (slot == (int)ctx->kry_hw - 1 && ctx->kry_born[slot] < 0)
      HIPCHK(hipMemsetAsync(ctx->KQ.p + (size_t)slot * ctx->ldq * qbytes(ctx), 0, (size_t)ctx->ldq * qbytes(ctx), st));
    const int m = (int)ctx->kry_hw;
    std::vector<double> htot(m, 0.0);
    double wn = 0.0, wr = 0.0, w0 = 0.0, w_first = 0.0;
    {
      // classical Gram-Schmidt; a second pass when the first one cancelled w by more than 1 / reorth.  With recycled
      // directions w = A M^-1 r lies mostly IN the kept space, so the usual 2x criterion fires on most iterations; the
      // orthogonality lost in one pass only matters relative to the tolerance asked for.
      // The update kernel reads the coefficients from device memory, so in a single context it is queued right behind
      // the product kernel and the host reads both results in one wait per pass (partitioned: the coefficients are
      // all-reduced by the host in between).  The phase timer brackets the kernels only, not the host's wait.
      double* hh_hot = hh + cap + 4;                 // second staging area of the pinned buffer (nh + 2 <= 34 values)
      int nh = 0;
      if (f32) {
        // exact (FP64) Gram-Schmidt against the window of this cycle's directions first;
        // columns [0, nh) of the window are in use (it fills from 0 and then turns into a ring)
        for (int k = 0; k < 32; ++k)
          if (ctx->hot_slots[k] >= 0) nh = k + 1;
        if (nh > 0) {
          {
            Phase ph(ctx, &ctx->t_ortho);
            launch_gcr_dots(st, false, ctx->KQh.p, ctx->ldq, n, nh, w, nullptr, ctx->scratch.p, ctx->hcoef_hot.p);
            if (!ctx->part)
              launch_gcr_axpy(st, false, ctx->KQh.p, ctx->ldq, n, nh, ctx->hcoef_hot.p, w, nullptr, ctx->scratch.p, ctx->gcr_out.p);
          }
          if (ctx->part) {
            FSICHK(gcr_read(ctx, ctx->hcoef_hot.p, nh + 2, hh_hot));
            FSICHK(allreduce(ctx, hh_hot, nh + 2));
            ctx->part_allreduces += 1;
            HIPCHK(hipMemcpyAsync(ctx->hcoef_hot.p, hh_hot, (size_t)nh * sizeof(double), hipMemcpyHostToDevice, st));
            Phase ph(ctx, &ctx->t_ortho);
            launch_gcr_axpy(st, false, ctx->KQh.p, ctx->ldq, n, nh, ctx->hcoef_hot.p, w, nullptr, ctx->scratch.p, ctx->gcr_out.p);
          } else {
            // read with the first pass below (stream order: the copy sees the values before hcoef_hot is reused)
            HIPCHK(hipMemcpyAsync(hh_hot, ctx->hcoef_hot.p, (size_t)(nh + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
          }
          ctx->ortho_q_cols += 2 * (int64_t)nh * 2; ctx->ortho_q_launches += 2;      // FP64 columns counted as two FP32 ones
        }
      }
      bool hot_pending = nh > 0;
      for (int pass = 0; pass < 2; ++pass) {
        double h2[2] = {0.0, 0.0};
        if (ctx->part) {
          // ONE all-reduce per pass while the basis is FP64: the m coefficients, |w|^2, w.r and - riding along - this rank's
          // part of |r|^2 as the previous iteration's update kernel left it (the exact norm of the residual this iteration
          // starts from).  What the update needs follows without a second reduction: |w'|^2 = |w|^2 - |h|^2 (the pass is
          // repeated when that cancels by more than 1 / reorth, and the repeat measures |w'|^2 directly), w'.r = w.r because
          // r is kept orthogonal to every q.  With an FP32 basis the identity is not good enough: the stored columns are
          // orthonormal to 1e-7 only, |w'|^2 comes out wrong by h^T (Q^T Q - I) h, the new column is then not a unit vector
          // and every later projection on it is off by that factor (measured: a 2-rank run lost a cycle and fell back to
          // FP64, a 1-rank run needed 184 instead of 50 iterations every other time) - so the FP32 basis pays a second,
          // two-number reduction for the exact |w'|^2 and w'.r after the update of w, as in round 2.
          {
            Phase ph(ctx, &ctx->t_ortho);
            launch_gcr_dots(st, f32, ctx->KQ.p, ctx->ldq, n, m, w, r, ctx->scratch.p, ctx->hcoef.p);
          }
          static const bool rccl_host = getenv("FSI_RCCL_HOST_REDUCE") != nullptr;      // debugging aid: stage the reductions through the host
          double exact2[2] = {0.0, 0.0};
          if (ctx->rccl && !rccl_host) {
            // the library's own communicator: the reductions run on the vectors where they are (device memory, solver stream)
            // and the update kernel is queued right behind them; the host reads the reduced numbers once per pass, for its
            // bookkeeping, exactly as in a single context
            if (rr_pending) HIPCHK(hipMemcpyAsync(ctx->hcoef.p + m + 2, ctx->gcr_out.p + 4, sizeof(double), hipMemcpyDeviceToDevice, st));
            else HIPCHK(hipMemsetAsync(ctx->hcoef.p + m + 2, 0, sizeof(double), st));
            FSICHK(rccl_allreduce_dev(ctx, ctx->hcoef.p, m + 3));
            {
              Phase ph(ctx, &ctx->t_ortho);
              launch_gcr_axpy(st, f32, ctx->KQ.p, ctx->ldq, n, m, ctx->hcoef.p, w, r, ctx->scratch.p, ctx->gcr_out.p + 2);
            }
            if (f32) {
              FSICHK(rccl_allreduce_dev(ctx, ctx->gcr_out.p + 2, 2));
              HIPCHK(hipMemcpyAsync(exact2, ctx->gcr_out.p + 2, sizeof exact2, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipMemcpyAsync(hh, ctx->hcoef.p, (size_t)(m + 3) * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
          } else {
            HIPCHK(hipMemcpyAsync(hh, ctx->hcoef.p, (size_t)(m + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
            if (rr_pending) HIPCHK(hipMemcpyAsync(hh + m + 2, ctx->gcr_out.p + 4, sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!rr_pending) hh[m + 2] = 0.0;
            FSICHK(allreduce(ctx, hh, m + 3));
            HIPCHK(hipMemcpyAsync(ctx->hcoef.p, hh, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
            {
              Phase ph(ctx, &ctx->t_ortho);
              launch_gcr_axpy(st, f32, ctx->KQ.p, ctx->ldq, n, m, ctx->hcoef.p, w, r, ctx->scratch.p, ctx->gcr_out.p + 2);
            }
            if (f32) {
              FSICHK(gcr_read(ctx, ctx->gcr_out.p + 2, 2, exact2));
              FSICHK(allreduce(ctx, exact2, 2));
            }
          }
          ctx->part_allreduces += f32 ? 2 : 1;
          if (rr_pending) { rn2 = hh[m + 2]; rr_pending = false; }      // exact |r|^2 before this iteration's update
          double hsq = 0.0;
          for (int j = 0; j < m; ++j) hsq += hh[j] * hh[j];
          h2[0] = f32 ? exact2[0] : std::max(hh[m] - hsq, 0.0);
          h2[1] = f32 ? exact2[1] : hh[m + 1];
          if (ctx->debug_gcr && *iters < 6)
            fprintf(stderr, "[gcr]   partitioned pass %d: |w|^2 %.6e |h|^2 %.6e w.r %.6e lagged |r|^2 %.6e window: nh %d |w|^2 %.6e\n", pass, hh[m], hsq,
                    hh[m + 1], hh[m + 2], nh, nh > 0 ? hh_hot[nh] : 0.0);
        } else {
          {
            Phase ph(ctx, &ctx->t_ortho);
            launch_gcr_dots(st, f32, ctx->KQ.p, ctx->ldq, n, m, w, nullptr, ctx->scratch.p, ctx->hcoef.p);
            launch_gcr_axpy(st, f32, ctx->KQ.p, ctx->ldq, n, m, ctx->hcoef.p, w, r, ctx->scratch.p, ctx->gcr_out.p);
          }
          HIPCHK(hipMemcpyAsync(hh, ctx->hcoef.p, (size_t)(m + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
          HIPCHK(hipMemcpyAsync(hh + m + 2, ctx->gcr_out.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
          HIPCHK(hipStreamSynchronize(st));
          h2[0] = hh[m + 2]; h2[1] = hh[m + 3];
        }
        if (hot_pending) {                       // the window's coefficients (read by the wait above, or all-reduced before)
          w0 = std::sqrt(std::max(hh_hot[nh], 0.0));
          for (int k = 0; k < nh; ++k)
            if (ctx->hot_slots[k] >= 0) htot[ctx->hot_slots[k]] += hh_hot[k];
          hot_pending = false;
        }
        if (pass == 0 && w0 == 0.0) w0 = std::sqrt(std::max(hh[m], 0.0));
        if (pass == 0) w_first = w0;
        for (int j = 0; j < m; ++j) htot[j] += hh[j];
        if (ctx->debug_gcr) {
          const double wref = std::sqrt(std::max(hh[m], 0.0));
          for (int j = 0; j < m; ++j) {
            const double a = std::fabs(hh[j]);
            ctx->dbg_cols += 1;
            if (a > 1e-6 * wref) ctx->dbg_sig6 += 1;
            if (a > 1e-9 * wref) ctx->dbg_sig9 += 1;
            if (a > 1e-12 * wref) ctx->dbg_sig12 += 1;
          }
        }
        if (ctx->debug_gcr && pass == 0 && h2[0] > 0.0) {
          // how many columns could have been left out of this pass with their part of w staying below 1 % of |w'| (1e-4 of |w'|^2)?
          std::vector<double> a2(m);
          for (int j = 0; j < m; ++j) a2[j] = hh[j] * hh[j];
          std::sort(a2.begin(), a2.end());
          double acc = 0.0; int drop = 0;
          for (int j = 0; j < m; ++j) { if (acc + a2[j] > 1e-4 * h2[0]) break; acc += a2[j]; drop += 1; }
          ctx->dbg_droppable += drop; ctx->dbg_drop_cols += m;
        }
        ctx->ortho_q_cols += 2 * (int64_t)m; ctx->ortho_q_launches += 2;
        wn = std::sqrt(std::max(h2[0], 0.0));
        wr = h2[1];
        // What one pass leaves of span(Q) in w' is (non-orthonormality of Q) x (cancellation |w| / |w'|), and that is the new
        // column's own error against the kept ones: with cancellations of 10 - 200 on most iterations a loose criterion lets
        // Q^T Q - I grow by that factor per column (measured on the avf problem, FP64 basis, second pass only beyond 100x:
        // 1.5e-4, 4e-3, then q_217 . q_221 = 1.0 - duplicate columns, |r| flat for 40 iterations at a time).  The pass itself
        // tells: |w'|^2 measured by the update kernel against |w|^2 - |h|^2, which differ by h^T (Q^T Q - I) h; their relative
        // difference over the cancellation estimates the error the new column would carry, and a second pass is made when
        // that exceeds the floor of the basis (FP64: 1e-9; FP32 columns are orthonormal to 6e-8 by storage: 3e-7 - scanned on the
        // 100-step run of the bench problem: 1e-5 and 1e-6 leave two fall-backs from the FP32 basis late in a Jacobian's life,
        // 3e-7 none, 13.1 against 12.2 - 12.35 Newton-it/s; the 20-step bench pays 0.6 %).
        bool lost = false;
        if (pass == 0 && (!ctx->part || f32) && h2[0] > 0.0 && hh[m] > 0.0) {
          double hsq2 = 0.0;
          for (int j = 0; j < m; ++j) hsq2 += hh[j] * hh[j];
          const double disc = std::fabs(h2[0] - (hh[m] - hsq2)) / h2[0];
          const double canc = std::sqrt(hh[m] / h2[0]);
          lost = disc / canc > (f32 ? ctx->orth_floor32 : ctx->orth_floor64);
          if (lost) ctx->gcr_reorth_forced += 1;
        }
        if (wn > reorth * w0 && !lost) break;
        w0 = wn;
      }
    }
    if (!(wn > 0.0) || !std::isfinite(wn)) {
      char buf[200];
      snprintf(buf, sizeof buf, "GCR breakdown (A M^-1 r vanished or is not finite): |w'| %.3e, |w| %.3e, w.r %.3e, %d kept, iteration %d", wn, w0, wr, m, *iters);
      ctx->err = buf;
      return FSI_ERR_LINEAR;
    }
    const double alpha = wr / wn;          // q . r with q = w / wn
    if (f32) {                              // the exact q goes into the FP64 window (ring of 32)
      qd = ctx->KQh.p + (size_t)ctx->hot_next * ctx->ldq;
      ctx->hot_slots[ctx->hot_next] = slot;
      ctx->hot_next = (ctx->hot_next + 1) % 32;
    }
    launch_gcr_update(st, f32, ctx->KQ.p, ctx->ldq, ctx->KZ.p, ctx->ldz, slot, n, w, z, 1.0 / wn, alpha, r, qd, ctx->scratch.p,
                      ctx->gcr_out.p + 4);
    src = r;
    // A direction that left the residual where it was (alpha^2 below 1e-3 |r|^2): A M^-1 r lies in the kept space, and as r
    // has not moved the next A M^-1 r is the same vector again - GCR proper cannot leave this point (seen on the 100 k-tet
    // mesh: |r| constant to four digits for 40 iterations until the stagnation rule ended the cycle, and again in the next
    // solve, which then lost the FP32 basis and the recycled space).  The next direction is made from the q just stored
    // instead (an Arnoldi step: the Krylov space of A M^-1 keeps growing whatever r does) until the residual moves again.
    if (alpha * alpha <= ctx->gcr_escape * rnorm * rnorm) { src = qd; ctx->gcr_arnoldi_steps += 1; }
    // coefficients of the new direction on the store:  p = (z - sum_j h_j p_j) / wn
    std::vector<double> c(cap, 0.0);
    c[slot] = 1.0;
    for (int j = 0; j < m; ++j) {
      const double hj = htot[j];
      if (hj == 0.0 || j == slot) continue;
      bool is_new = false;
      for (size_t k = 0; k < cy.slots.size(); ++k)
        if (cy.slots[k] == j) {                 // a direction of this cycle: expand it on the store
          for (int64_t i = 0; i < cap; ++i) c[i] -= hj * cy.cn[k][i];
          is_new = true;
          break;
        }
      if (!is_new) c[j] -= hj;
    }
    for (auto& v : c) v /= wn;
    for (int64_t i = 0; i < cap; ++i) cy.y[i] += alpha * c[i];
    cy.cn.push_back(std::move(c));
    cy.slots.push_back(slot);
    ctx->kry_born[slot] = ctx->kry_m;
    ctx->kry_m += 1;
    *iters += 1;
    ctx->kry_iters += 1;
    // |r|: the recurrence value; read back (it is one host wait, shared with nothing else) because the analytic
    // |r|^2 - alpha^2 loses its digits exactly when the iteration converges fast
    if (ctx->part) {
      // |r'|^2 = |r|^2 - alpha^2 from the exact |r|^2 this iteration started with; the exact value of |r'|^2 (this rank's
      // part is in gcr_out[4]) travels with the next pass's reduction.  Only an iteration that looks converged pays a
      // reduction of its own, to be sure.
      rn2 = std::max(rn2 - alpha * alpha, 0.0);
      rr_pending = true;
      if (std::sqrt(rn2) <= target || !std::isfinite(rn2)) {
        FSICHK(gcr_read(ctx, ctx->gcr_out.p + 4, 1, hh));
        FSICHK(allreduce(ctx, hh, 1));
        ctx->part_allreduces += 1;
        rn2 = hh[0];
        rr_pending = false;
      }
      rnorm = std::sqrt(std::max(rn2, 0.0));
    } else {
      FSICHK(gcr_read(ctx, ctx->gcr_out.p + 4, 1, hh));
      rnorm = std::sqrt(std::max(hh[0], 0.0));
    }
    if (ctx->debug_gcr && getenv("FSI_DEBUG_GCR_ALL"))
      fprintf(stderr, "[gcr]     it %d: |w'|/|w| %.2e alpha/|r| %.2e |r| %.4e%s\n", *iters, wn / std::max(w_first, 1e-300), alpha / std::max(rnorm, 1e-300), rnorm, src == r ? "" : " (next from q)");
    if (ctx->debug_gcr && (*iters % 10 == 0)) {
      fprintf(stderr, "[gcr] it %d |r| %.3e target %.3e m %d  |h_j| > 1e-6/1e-9/1e-12 |w|: %.2f %.2f %.2f of the columns\n", *iters, rnorm, target, m,
              (double)ctx->dbg_sig6 / std::max<int64_t>(1, ctx->dbg_cols), (double)ctx->dbg_sig9 / std::max<int64_t>(1, ctx->dbg_cols),
              (double)ctx->dbg_sig12 / std::max<int64_t>(1, ctx->dbg_cols));
      fprintf(stderr, "[gcr]   columns whose coefficients together stay below 1 %% of |w'|: %.3f of the kept ones\n", (double)ctx->dbg_droppable / std::max<int64_t>(1, ctx->dbg_drop_cols));
      fflush(stderr);
    }
    if (!std::isfinite(rnorm)) { ctx->err = "GCR diverged (non-finite residual)"; return FSI_ERR_LINEAR; }
    if (rnorm < 0.9 * best) { best = rnorm; since_gain = 0; } else since_gain += 1;
    if ((int)cy.slots.size() == 32) FSICHK(gcr_flush(ctx, cy, x));
  }
  FSICHK(gcr_flush(ctx, cy, x));
  *rnorm_out = rnorm;
  return FSI_OK;
}

}  // namespace

namespace fsi {
namespace host {

int solve_gcr(FsiCtx* ctx, const double* rhs, double* x, double rtol_in, int max_it, int* iters, double* relres) {
  double rtol = rtol_in;           // tightened below when an adaptive solve (ctx->utol) leaves too much in the unscaled norm
  const int64_t n = ctx->ndof;
  hipStream_t st = ctx->stream;
  double* r = ctx->tmp1.p;
  launch_copy(st, r, rhs, n);
  launch_fill(st, x, n, 0.0);
  double bnorm = 0.0, rnorm = 0.0;
  FSICHK(gnorm2(ctx, r, &bnorm));
  *iters = 0;
  if (bnorm == 0.0) { *relres = 0.0; return FSI_OK; }
  if (!std::isfinite(bnorm)) { ctx->err = "non-finite right-hand side"; return FSI_ERR_LINEAR; }
  // Storage of Q for this Jacobian's lifetime, decided by the first solve after the refresh: FP32 (half the dominant
  // stream, exact FP64 window for the directions of the current cycle, restart from the true residual) when the accuracy
  // that may be asked for during the lifetime leaves room for it.  Inside fsi_newton_solve that is the floor of the
  // forcing term at the largest right-hand side seen so far (tol_hint); the inexact-Newton tolerances of a production run
  // qualify (5e-7 on the bench), the parity tests that drive Newton to round-off keep FP64.
  if (ctx->kry_hw == 0 && ctx->kry_fp32_policy == 3) ctx->kry_fp32 = 0;
  if (ctx->kry_hw == 0 && ctx->kry_fp32_policy == 2) {
    const double lowest = ctx->tol_hint > 0.0 ? std::min(ctx->tol_hint, rtol) : rtol;
    ctx->kry_fp32 = lowest > ctx->tune.krylov_fp32_floor;
  }
  // adaptive solve: start where the last check under this Jacobian says the unscaled criterion will be met (a re-entered cycle
  // costs a projection on the kept space and a flush - three passes over the store - so guessing right the first time matters)
  if (ctx->utol > 0.0 && ctx->utol_ratio > 0.0 && rtol > ctx->utol_rtol_floor)
    rtol = std::max(ctx->utol_rtol_floor, std::min(rtol, 0.7 * ctx->utol / ctx->utol_ratio));
  // the kept directions serve every later solve with this matrix, so the tightest tolerance asked for since the refresh
  // decides the re-orthogonalisation criterion, not this solve's
  ctx->gs_rtol = ctx->gs_rtol > 0.0 ? std::min(ctx->gs_rtol, rtol) : rtol;
  double rstart = bnorm;
  rnorm = bnorm;
  auto true_residual = [&]() -> int {
    FSICHK(halo_update(ctx, x));
    FSICHK(spmv(ctx, x, ctx->tmp3.p));
    zero_ghost(ctx, ctx->tmp3.p);
    launch_axpby(st, r, 1.0, rhs, -1.0, ctx->tmp3.p, n);
    return gnorm2(ctx, r, &rnorm);
  };
  int stalls = 0;
  bool near_ok = false;
  const int64_t cap_now = ctx->kry_cap;
  for (int tighten = 0; tighten < 8; ++tighten) {
  for (int cyc = 0; cyc < 8 && *iters < max_it; ++cyc) {
    // FP32 storage of Q: the residual recurrence of one cycle is good to about 1e-6 of the residual the cycle started from;
    // a tighter request is met by restarting the cycle from the true residual b - A x (iterative refinement).  With the FP32
    // copy of the matrix in the iterations every answer is judged on the residual of the FP64 matrix before it is returned
    // (one FP64 product per cycle); without it, every answer asked for below 1e-4
    const bool f32 = ctx->kry_fp32 != 0;
    // (measured on the bench workload, round 3: at a recurrence residual of 6e-6 |b| the true one differs in the third digit,
    // at 1e-2 not in the fourth; the first solve on a fresh FP32 store is the exception - 6e-5 against 4e-4 - and the
    // verdict below catches it.  A cycle may therefore run down to 1e-6 of its start; round 2's 1e-5 cost every first solve
    // of a time step - tolerances of 3e-6 .. 9e-6 - a second cycle: one more FP64 product and two passes over Q.)
    const double target = f32 ? std::max(rtol * bnorm, ctx->f32_cycle_floor * rstart) : rtol * bnorm;
    const int its0 = *iters;
    FSICHK(gcr_cycle(ctx, r, x, target, ctx->gs_rtol, max_it, iters, &rnorm));
    if (!f32) {
      // FP64 basis.  The recurrence residual is only as good as the kept pairs: x is built from the directions p_k, the
      // recurrence from q_k, and A p_k = q_k holds to round-off TIMES what the recursion p_k = (z_k - sum_j h_jk p_j) / |w'|
      // has amplified - measured on the known-answer case driven to 1e-11: 1e-9 for the pairs of a fresh Jacobian, 5e-6 within
      // 33 directions of a hard solve (every step cancelling w a hundredfold), 1e+2 a Jacobian lifetime later, with the
      // recurrence reporting 1e-11 all along.  So the answer of every cycle is judged on b - A x with the FP64 matrix (one
      // product, as the FP32 basis always did), the next cycle starts from that residual (iterative refinement over the
      // pairs' inconsistency), and a cycle that does not halve the true residual means the kept pairs are no longer pairs:
      // they are dropped.
      //
      // When the verdict is taken: always for tight answers (below 1e-8), after anything that has shown the pairs at risk - a
      // fall-back from the FP32 basis in this Jacobian's life, a full (rotating) store, a cycle of more than 64 iterations, a
      // stalled or stagnated cycle, an earlier verdict of this store that differed from its recurrence by more than a tenth
      // of the tolerance - and on the first cycle's answer otherwise NOT: with a fresh Jacobian, a growing store and loose
      // tolerances (the all-FP64-storage production runs: 1e-5 .. 1e-2) the pairs hold to 1e-9 (measured), the FP64
      // operator is the one the iterations ran on, and the product is 2.7 % of such a run.
      const bool at_risk = rtol < 1e-8 || ctx->kry_fp32_policy == 3 || (ctx->kry_hw == cap_now && ctx->kry_free.empty()) ||
                           *iters - its0 > 64 || ctx->gcr_stalled || ctx->gcr_stagnated || ctx->f64_suspect || cyc > 0 ||
                           rnorm > rtol * bnorm;
      if (!at_risk) break;
      const double rec64 = rnorm;
      FSICHK(true_residual());
      if (std::fabs(rnorm - rec64) > 0.1 * rtol * bnorm) ctx->f64_suspect = true;
      if (rnorm <= rtol * bnorm) break;
      // attainable accuracy: a tolerance at round-off level (1e-11 on a system with the 1e7 penalty rows) may be met by the
      // recurrence and missed by a factor of a few by b - A x; a second verified cycle that is still within 100x is as good
      // as FP64 makes it, and Newton's own residual check judges the step
      if (rtol <= 1e-9 && rnorm <= 100.0 * rtol * bnorm && (ctx->gcr_stagnated || cyc >= 1)) { near_ok = true; break; }
      if (*iters >= max_it) break;
      if (ctx->gcr_stalled || !(rnorm < 0.5 * rstart)) {      // (stalled: the truncated recurrence of a full store made no progress)
        if (stalls >= 2) break;
        stalls += 1;
        ctx->gcr_restarts += 1;
        gcr_reset(ctx);                      // x keeps what the flushed directions gave it
      }
      rstart = rnorm;
      continue;
    }
    const bool final_cycle = target <= rtol * bnorm * (1.0 + 1e-12);
    if (final_cycle && rtol >= 1e-4 && !ctx->op32_ok) break;
    // A loose answer (the later Newton iterations of a step ask for 1e-3 .. 1e-2; 38 of the bench's 58 solves, 2.65 ms of FP64
    // product each): recurrence and truth agree to three digits and better there (every FP32 cycle of the bench and of the avf
    // runs, once the kept columns stay orthonormal - the first attempt at this skip met a solve that reported 1e-2 with a
    // true residual of 1.7 |b|: duplicate columns, see the orthogonality criterion in gcr_cycle), and the next thing that
    // happens is Newton's assembly of the FP64 residual from the updated state, the judge of the step either way.  Skipped
    // only while the LAST VERIFIED cycle on this store found recurrence and truth closer than 1 % of what is asked now, the
    // new directions all sat in the exact FP64 window and nothing stagnated.
    // Only inside fsi_newton_solve (in_newton): there the FP64 residual assembled from the updated state follows and judges the
    // step.  A direct fsi_solve caller has no such judge, so its answers always get the FP64 verdict and `relres`
    // is the true residual; when verdicts_skipped counts up, the FsiNewtonIter.lin_relres of that iteration is the recurrence value.
    if (ctx->in_newton && final_cycle && rtol >= ctx->f32_verdict_skip_rtol && rnorm <= rtol * bnorm && *iters - its0 <= 32 && !ctx->gcr_stagnated &&
        ctx->f32_last_drift >= 0.0 && ctx->f32_last_drift <= 0.01 * rtol) {
      ctx->verdicts_skipped += 1;
      break;
    }
    const double rec32 = rnorm;
    FSICHK(true_residual());
    ctx->f32_last_drift = std::fabs(rnorm - rec32) / bnorm;
    if (getenv("FSI_DEBUG_TRUERES"))
      fprintf(stderr, "[gcr]   fp32 cycle %d: recurrence |r|/|b| %.3e (target %.3e), true %.3e, rtol %.1e, its %d\n", cyc, rec32 / bnorm, target / bnorm, rnorm / bnorm, rtol, *iters);
    if (rnorm <= rtol * bnorm) break;
    if (!(rnorm < 0.5 * rstart)) {
      // the cycle did not bring the true residual down: FP32 storage has lost this system (a tolerance near round-off,
      // or a cancellation the FP64 window did not cover).  Drop the kept directions and finish in FP64 from here.
      if (ctx->kry_fp32_policy == 1) {
        // FSI_KRYLOV_FP32=1 sized the basis store for 4-byte columns: there is no FP64 store to fall back to, and
        // addressing it with 8-byte columns would run past the allocation.  The policy was forced, so say so.
        char buf[200];
        snprintf(buf, sizeof buf, "GCR: the FP32 Krylov basis forced by FSI_KRYLOV_FP32=1 cannot reach rtol %.1e on this system "
                 "(true residual %.3e of |b| after a cycle); use the default policy", rtol, rnorm / bnorm);
        ctx->err = buf;
        *relres = rnorm / bnorm;
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
    }
    rstart = rnorm;
  }
  // adaptive Newton solves: the unscaled residual D_r^-1 r against utol |b| (r: the residual the cycles ended on)
  if (!(ctx->utol > 0.0) || !(rnorm <= rtol * bnorm) || rtol <= ctx->utol_rtol_floor * (1.0 + 1e-12) || *iters >= max_it) break;
  double ru = 0.0;
  launch_div(st, ctx->tmp3.p, r, ctx->rowscale.p, n);
  FSICHK(gnorm2(ctx, ctx->tmp3.p, &ru));
  if (rnorm > 0.0 && ctx->b_unscaled > 0.0) ctx->utol_ratio = (ru / ctx->b_unscaled) / (rnorm / bnorm);
  if (!(ru > ctx->utol * ctx->b_unscaled)) break;
  const double want = 0.5 * ctx->utol * ctx->b_unscaled / ru;              // aim a factor two below
  rtol = std::max(ctx->utol_rtol_floor, rtol * std::min(0.5, std::max(0.02, want)));
  ctx->utol_tightened += 1;
  rstart = rnorm;
  }
  *relres = rnorm / bnorm;
  if (getenv("FSI_DEBUG_TRUERES")) {
    const double rec = rnorm;
    FSICHK(true_residual());
    fprintf(stderr, "[gcr] solve: %d its, recurrence |r|/|b| %.3e, true %.3e, kept %lld (hw %lld), restarts %lld, basis fp%d policy %d, rtol %.1e gs_rtol %.1e |b| %.3e\n", *iters, rec / bnorm, rnorm / bnorm,
            (long long)(ctx->kry_hw - (int64_t)ctx->kry_free.size()), (long long)ctx->kry_hw, (long long)ctx->gcr_restarts, ctx->kry_fp32 ? 32 : 64, ctx->kry_fp32_policy, rtol, ctx->gs_rtol, bnorm);
    rnorm = rec;
    if (!ctx->kry_fp32 && ctx->kry_hw > 0) {      // A p_k = q_k for the kept pairs?
      double worst = 0.0; int64_t wk = -1; double qn_w = 0.0;
      for (int64_t k = 0; k < ctx->kry_hw; ++k) {
        if (ctx->kry_born[k] < 0) continue;
        FSICHK(spmv(ctx, ctx->KZ.p + (size_t)k * ctx->ldz, ctx->tmp3.p));
        const double* qk = reinterpret_cast<const double*>(ctx->KQ.p) + (size_t)k * ctx->ldq;
        launch_axpby(st, ctx->tmp3.p, 1.0, ctx->tmp3.p, -1.0, qk, n);
        double e = 0.0, qn = 0.0;
        FSICHK(dot_n(ctx, ctx->tmp3.p, ctx->tmp3.p, n, &e));
        FSICHK(dot_n(ctx, qk, qk, n, &qn));
        const double rel = std::sqrt(e / std::max(qn, 1e-300));
        if (rel > worst) { worst = rel; wk = k; qn_w = qn; }
        if (rel > 1e-9) fprintf(stderr, "[gcr]     slot %lld born %lld: |A p - q|/|q| %.3e |q| %.6f\n", (long long)k, (long long)ctx->kry_born[k], rel, std::sqrt(qn));
      }
      fprintf(stderr, "[gcr]   worst pair: slot %lld |A p - q|/|q| %.3e (|q| %.6f)\n", (long long)wk, worst, std::sqrt(qn_w));
      // orthonormality of the kept columns: rows of Q^T Q for the last few slots
      const int mm = (int)ctx->kry_hw;
      double worst_o = 0.0; int wi = -1, wj = -1;
      for (int j = std::max(0, mm - 6); j < mm; ++j) {
        if (ctx->kry_born[j] < 0) continue;
        const double* qj = reinterpret_cast<const double*>(ctx->KQ.p) + (size_t)j * ctx->ldq;
        launch_gcr_dots(st, false, ctx->KQ.p, ctx->ldq, n, mm, qj, nullptr, ctx->scratch.p, ctx->hcoef.p);
        FSICHK(gcr_read(ctx, ctx->hcoef.p, mm + 2, ctx->gcr_host));
        for (int i = 0; i < mm; ++i) {
          if (ctx->kry_born[i] < 0) continue;
          const double dev = std::fabs(ctx->gcr_host[i] - (i == j ? 1.0 : 0.0));
          if (dev > worst_o) { worst_o = dev; wi = i; wj = j; }
        }
      }
      fprintf(stderr, "[gcr]   orthonormality of the last columns: max |q_i . q_j - delta| = %.3e (i %d, j %d)\n", worst_o, wi, wj);
    }
  }
  // stagnation within a factor 100 of a tolerance below 1e-9 (after the restarts above): the answer is as accurate as FP64 makes it on this system, and
  // the caller (Newton's own residual check) judges the step; reported through relres
  if ((near_ok || ctx->gcr_stagnated) && rtol <= 1e-9 && rnorm <= 100.0 * rtol * bnorm) return FSI_OK;
  if (!(rnorm <= rtol * bnorm)) {
    char buf[160];
    snprintf(buf, sizeof buf, "GCR: no convergence in %d iterations (relres %.3e, tol %.1e)", *iters, *relres, rtol);
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
