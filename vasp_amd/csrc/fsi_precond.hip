// The field-split block preconditioner of the monolithic Jacobian: one application (precondition_block: ~210 dependent
// launches on two HIP streams) and its refresh at every new Jacobian (refresh_preconditioner: field blocks, explicit Schur
// complement, Galerkin coarse operators, eigenvalue estimates, self-test).  Kernels: fsi_block.hip.  DESIGN.md section 5.
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace {

// Chebyshev solve of the masked velocity block (see fsi_block.hip); W: 2 work vectors (r, t) + d
struct CsrRef { int64_t n; const int64_t* rowptr; const int32_t* cols; const double* vals; const int64_t* diagpos; };
// Chebyshev solve with a Jacobi scaling taken from (dvals, diagpos); `apply(in, out)` is the operator. W: 3 work vectors.
template <class Apply>
void cheb_solve_op(FsiCtx* ctx, int64_t n, Apply&& apply, const double* dvals, const int64_t* diagpos, const double* mask,
                   const double* rhs, double* x, double* W, int its, double lmax, double kappa) {
  hipStream_t st = ctx->stream;
  double *r = W, *d = W + n, *t = W + 2 * n;
  const double lmin = lmax / kappa, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
  double rho = 1.0 / sig;
  launch_cheb_init(st, n, mask, rhs, diagpos, dvals, 1.0 / th, x, r, d);
  for (int k = 0; k < its; ++k) {
    apply(d, t);
    const double rn = 1.0 / (2.0 * sig - rho);
    launch_cheb_step(st, n, mask, t, diagpos, dvals, rn * rho, 2.0 * rn / de, x, r, d);
    rho = rn;
  }
}
void cheb_solve(FsiCtx* ctx, const CsrRef& M, const double* mask, const double* rhs, double* x, double* W, int its,
                double lmax, double kappa) {
  cheb_solve_op(ctx, M.n, [&](const double* in, double* out) { launch_spmv(ctx->stream, M.n, M.rowptr, M.cols, M.vals, in, out); },
                M.vals, M.diagpos, mask, rhs, x, W, its, lmax, kappa);
}
CsrRef vv_ref(FsiCtx* c) { return CsrRef{3 * c->N2, c->rowptr3.p, c->cols3.p, c->Mvv.vals.p, c->diagpos3.p}; }
CsrRef ss_ref(FsiCtx* c) { return CsrRef{3 * c->nS, c->ss_rowptr.p, c->ss_cols.p, c->ss_vals.p, c->ss_diagpos.p}; }
// largest eigenvalue of mask D^-1 A mask by power iteration from a pseudo-random start (rich in element-scale modes)
template <class Apply>
int power_lmax_op(FsiCtx* ctx, int64_t n, Apply&& apply, const double* dvals, const int64_t* diagpos, const double* mask,
                  double* W, double* out) {
  hipStream_t st = ctx->stream;
  double *x = W, *y = W + n;
  launch_mask_ripple(st, n, mask, x);
  double lam = 1.0;
  for (int k = 0; k < 40; ++k) {
    apply(x, y);
    launch_mask_scale(st, n, mask, diagpos, dvals, y);
    double xx = 0.0, yy = 0.0;
    FSICHK(dot_n(ctx, x, x, n, &xx));
    FSICHK(dot_n(ctx, y, y, n, &yy));
    if (!(xx > 0.0) || !(yy > 0.0) || !std::isfinite(yy)) break;
    lam = std::sqrt(yy / xx);
    launch_copy(st, x, y, n);
    launch_scale(st, x, 1.0 / std::sqrt(yy), n);
  }
  *out = 1.2 * lam;
  return FSI_OK;
}
int power_lmax(FsiCtx* ctx, const CsrRef& M, const double* mask, double* W, double* out) {
  return power_lmax_op(ctx, M.n, [&](const double* in, double* o) { launch_spmv(ctx->stream, M.n, M.rowptr, M.cols, M.vals, in, o); },
                       M.vals, M.diagpos, mask, W, out);
}
// Schur operator y = (A_pp - Apv~ D^-1 A_vp) x ; w3: work vector of length 3 N2
void schur_apply(FsiCtx* ctx, const double* in, double* out, double* w3) {
  (void)w3;
  launch_spmv(ctx->stream, ctx->V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals.p, in, out, SPMV_FIELD_BLOCK);
}

// The last sweep of a Chebyshev chain is not launched.  A sweep does  x += d_in;  r -= A d_in;  d_out = c1 d_in + c2 B^-1 r,
// and what follows a chain reads x alone: the last product feeds only an r and a d that nobody reads.  The chain's consumer
// takes x and the current direction and forms x + d itself, the same addition in the same precision (fsi_block.hip,
// k_unpad_from_f32), so an application's output keeps its bits.  FsiTuning.experiment bit 2 launches every sweep as before.
inline bool drop_last_sweep(const FsiCtx* ctx) { return (ctx->tune.experiment & 4) == 0; }

// FP32 Chebyshev sweeps on a component-diagonal node-block matrix; dinv carries the Jacobi scaling and the mask.
// Returns the number of product sweeps launched.
int cheb_db_f32(FsiCtx* ctx, const float* db, const float* dinv, const double* rhs, double* x, double* W, int its,
                 double lmax, double kappa, hipStream_t st = nullptr) {
  const int64_t n = 4 * ctx->N2;                 // float4 per node
  if (!st) st = ctx->stream;
  float* F = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(W) + 15) & ~uintptr_t(15));   // float4 loads
  float *fr = F, *fd = F + n, *ft = F + 2 * n, *fx = F + 3 * n, *frhs = F + 4 * n;
  const double lmin = lmax / kappa, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
  double rho = 1.0 / sig;
  (void)frhs;
  const int launched = (its > 0 && drop_last_sweep(ctx)) ? its - 1 : its;      // without the chain's last sweep: the unpad adds its d
  launch_pad_init_f32(st, ctx->N2, rhs, nullptr, dinv, (float)(1.0 / th), fx, fr, fd);      // pad + initialise in one launch
  if (ctx->tiled && ctx->fused_sweeps) {
    float *da = fd, *db_ = ft;                   // d is ping-ponged; the product stays in registers
    for (int k = 0; k < launched; ++k) {
      const bool timed = ctx->sample_budget > 0 && k < 4 && ctx->db_ev0[0] && ctx->db_samples_pending < 8;
      if (timed) (void)hipEventRecord(ctx->db_ev0[ctx->db_samples_pending], st);
      const double rn = 1.0 / (2.0 * sig - rho);
      if (ctx->sweeps_fp16 && db == ctx->vv_db32.p)
        launch_sweep_tiled_h(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->vv_rec.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr,
                             dinv, (float)(rn * rho), (float)(2.0 * rn / de), da, db_, fx, fr);
      else if (ctx->vv_rec32.p && db == ctx->vv_db32.p)
        launch_sweep_tiled_r3(st, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->vv_rec32.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr,
                             dinv, (float)(rn * rho), (float)(2.0 * rn / de), da, db_, fx, fr);
      else
        launch_sweep_tiled_f32(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, db, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                               nullptr, dinv, (float)(rn * rho), (float)(2.0 * rn / de), da, db_, fx, fr);
      if (timed) { (void)hipEventRecord(ctx->db_ev1[ctx->db_samples_pending], st); ctx->db_samples_pending += 1; }
      std::swap(da, db_);
      rho = rn;
    }
    launch_unpad_from_f32(st, ctx->N2, fx, x, launched < its ? da : nullptr);
    return launched;
  }
  for (int k = 0; k < launched; ++k) {
    const bool timed = ctx->sample_budget > 0 && k < 4 && ctx->db_ev0[0] && ctx->db_samples_pending < 8;
    if (timed) (void)hipEventRecord(ctx->db_ev0[ctx->db_samples_pending], st);
    if (ctx->tiled)
      launch_spmv_tiled_f32(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, db, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr, fd, ft);
    else
      launch_spmv_db_f32(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, db, fd, ft);
    if (timed) { (void)hipEventRecord(ctx->db_ev1[ctx->db_samples_pending], st); ctx->db_samples_pending += 1; }
    const double rn = 1.0 / (2.0 * sig - rho);
    launch_cheb_step_f32(st, n, ft, dinv, (float)(rn * rho), (float)(2.0 * rn / de), fx, fr, fd);
    rho = rn;
  }
  launch_unpad_from_f32(st, ctx->N2, fx, x, launched < its ? fd : nullptr);
  return launched;
}

// z = M^-1 r with the approximate block factorisation (see fsi_block.hip):  (v,p) by SIMPLE with the d-eliminated
// velocity block, then d.
}  // namespace

namespace fsi {
namespace host {

int precondition_block(FsiCtx* ctx, const double* r, double* z) {
  const int64_t n3 = 3 * ctx->N2, V = ctx->V, N2 = ctx->N2;
  hipStream_t st = ctx->stream;
  double* W = ctx->blk.p;
  double *rd = W, *rv = W + n3, *rp = W + 2 * n3, *vs = W + 3 * n3, *tp = W + 4 * n3, *dp = W + 5 * n3, *dv = W + 6 * n3,
         *td = W + 7 * n3, *dd = W + 8 * n3, *IW = W + 9 * n3, *w3 = W + 19 * n3;     // IW: 10 vectors; its first 4 hold the (FP32, float4-padded) sweep work
  // Two chains side by side (prec_streams; default configuration only: FP32 solid cycle, FP32 fluid sweeps, FP16 / FP32 Schur
  // sweeps with FP64 vectors, scalar displacement block).  The application is a chain of ~210 dependent launches, most of them
  // short of filling the chip (latency- and issue-bound sweeps on 0.1 - 0.6 GB of data), and its dependences are fewer than
  // its order: the fluid predictor does not need the solid one (block Jacobi instead of Gauss-Seidel between the two parts:
  // same Krylov counts, measured), and the displacement block needs the velocity on the SOLID rows only, where the pressure
  // correction is small (dd_early: measured).  Stream A (the solver stream): split, solid predictor, displacement block,
  // merge.  Stream B: fluid predictor, then - once the solid predictor is there - pressure right-hand side, Schur sweeps,
  // velocity correction.  Work vectors of the two chains are disjoint: the solid and displacement sweeps use IW[0, 4 n3),
  // the fluid sweeps IW[6 n3, 10 n3), the Schur sweeps the unused tail of rp (V of its n3 entries carry r_p).
  const bool conc = ctx->prec_streams && ctx->stream2 && ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused && ctx->sbmg_ready &&
                    ctx->sweeps_fp32 && ctx->tiled && ctx->fused_sweeps && ctx->cheb_its_p > 0 &&
                    ((ctx->schur_fp32 == 1 && ctx->s_vals32.p) || ctx->schur_fp32 == 0) &&      // (round 5: also with the all-FP64 Schur sweeps - the FP64-storage mode ran its ~5 ms application as ONE chain)
                    ctx->pv32_ok && ctx->adv_is_db && ctx->cheb_its_d > 0 && ctx->dd_is_scalar && 4 * V <= n3 && ctx->debug_prec_apply == 0;
  // (the applications whose sweep launches are timed by event pairs issue both chains on the solver stream - the same arithmetic in
  // the same order per chain, and a pair brackets its kernel alone)
  hipStream_t sA = ctx->stream, sB = (conc && ctx->sample_budget <= 0) ? ctx->stream2 : ctx->stream;
  const bool drop = drop_last_sweep(ctx);      // every chain below ends one sweep early and hands its consumer x and d
  int sweeps_f = 0;                            // product sweeps launched by the fluid predictor
  launch_split(st, N2, V, r, rd, rv, rp);
  if (conc) { HIPCHK(hipEventRecord(ctx->ev_split, sA)); HIPCHK(hipStreamWaitEvent(sB, ctx->ev_split, 0)); }
  // velocity predictor: block Gauss-Seidel solid (elasticity-dominated, many cheap sweeps) -> fluid interior (mass-dominated)
  {
    double *xs = IW + 4 * n3, *xf = IW + 5 * n3, *rhs2 = IW + 6 * n3;
    double *cs_rhs = IW + 7 * n3, *cs_x = IW + 8 * n3;            // compact solid vectors (3 nS <= n3)
    if (conc)      // stream B, issued first: the fluid predictor straight from r_v (no coupling to the solid predictor), work area IW[6 n3, 10 n3)
      sweeps_f = cheb_db_f32(ctx, ctx->vv_db32.p, ctx->vvf_dinv32.p, rv, xf, IW + 6 * n3, ctx->cheb_its_f, ctx->lmax_f, ctx->cheb_kappa_f, sB);
    if (ctx->solid_fp32) {
      const int64_t n = 4 * ctx->nS;               // float4 per solid node
      float* F = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(IW) + 15) & ~uintptr_t(15));   // float4 loads
      float *fr = F, *fd = F + n, *ft = F + 2 * n, *fx = F + 3 * n, *frhs = F + 4 * n;
      const double lmax = ctx->lmax_s, lmin = lmax / ctx->cheb_kappa_s, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
      double rho = 1.0 / sig;
      const bool bj = ctx->solid_block_jacobi != 0;
      const bool fused = bj && ctx->solid_fused;
      const bool cycle = fused && ctx->sbmg_ready;      // the two-level cycle: gather, x = 0, first direction and the zeroed second buffer in ONE launch below
      if (!cycle) launch_gather3_f32(st, ctx->nS, ctx->snode.p, rv, frhs);
      if (cycle) {}
      else if (bj) launch_cheb_init_b3(st, ctx->nS, frhs, ctx->sb_binv12.p, (float)(1.0 / th), fx, fr, fd);
      else launch_cheb_init_f32(st, n, frhs, ctx->sb_dinv.p, (float)(1.0 / th), fx, fr, fd);
      if (fused && !cycle) HIPCHK(hipMemsetAsync(ft, 0, n * sizeof(float), st));     // second d buffer (ping-pong), pads stay zero
      float *dcur = fd, *dnext = ft;
      const float* xs_d = nullptr;                 // the direction the scatter below adds to fx: that of the dropped last sweep
      if (fused && ctx->sbmg_ready) {
        // two-level cycle (see the displacement block): smoothing on [lmax/alpha, lmax], coarse solve on the solid vertices
        const double slmin = lmax / ctx->sbmg_alpha, sth = 0.5 * (lmax + slmin), sde = 0.5 * (lmax - slmin), ssig = sth / sde;
        double srho = 1.0 / ssig;
        // FSI_CHEB4 bit 0: the smoothing sweeps as Chebyshev polynomials of the 4th kind (Lottes 2022: the smoother that
        // minimises the two-level bound for a given degree; needs lmax only):  d_0 = 4/(3 lmax) B^-1 r,
        // d_i = (2i-1)/(2i+3) d_{i-1} + (8i+4)/((2i+3) lmax) B^-1 r_i
        const bool s4 = (ctx->cheb4 & 1) != 0;
        const double sinit = s4 ? 4.0 / (3.0 * lmax) : 1.0 / sth;
        auto s4c = [&](int i, float* c1, float* c2) { *c1 = (float)((2.0 * i - 1.0) / (2.0 * i + 3.0)); *c2 = (float)((8.0 * i + 4.0) / ((2.0 * i + 3.0) * lmax)); };
        launch_solid_cycle_init(st, ctx->nS, ctx->snode.p, rv, ctx->sb_binv12.p, (float)sinit, fx, fr, fd, ft);
        auto sweep = [&](float c1, float c2, int sample) {
          const bool timed = ctx->sample_budget > 0 && sample >= 0 && sample < 8 && ctx->ss_ev0[0];
          if (timed) (void)hipEventRecord(ctx->ss_ev0[sample], st);
          if (ctx->sweeps_fp16 && ctx->sb_rec.p)
            launch_sweep_sb_h(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_rec.p, ctx->sb_binv12.p, c1, c2, dcur, dnext, fx, fr);
          else if (ctx->sb_rec32.p)
            launch_sweep_sb_r(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_rec32.p, ctx->sb_binv12.p, c1, c2, dcur, dnext, fx, fr);
          else
            launch_sweep_sb_b3(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, ctx->sb_binv12.p, c1, c2, dcur, dnext, fx, fr);
          if (timed) (void)hipEventRecord(ctx->ss_ev1[sample], st);
          std::swap(dcur, dnext);
        };
        for (int k = 0; k < ctx->sbmg_pre; ++k) {
          if (s4) { float c1, c2; s4c(k + 1, &c1, &c2); sweep(c1, c2, k); continue; }
          const double rn = 1.0 / (2.0 * ssig - srho);
          sweep((float)(rn * srho), (float)(2.0 * rn / sde), k);
          srho = rn;
        }
        const int64_t nc = ctx->sbmg_nc, n4c = 4 * nc;
        float *cr = ctx->sbmg_work.p, *cd = cr + n4c, *cd2 = cr + 2 * n4c, *cx = cr + 3 * n4c, *crhs = cr + 4 * n4c;
        const bool exact = bcr_ready(ctx);
        const float* cx_d = nullptr;                // the coarse chain's direction, when its last sweep is dropped
        launch_sbmg_restrict(st, nc, ctx->sbmg_chptr.p, ctx->sbmg_child.p, ctx->sbmg_chw.p, ctx->snode.p, ctx->rowscale.p,
                             ctx->sbmg_flag.p, ctx->sbmg_cflag.p, fr, crhs, exact ? bcr_pos(ctx) : nullptr, exact ? bcr_rhs(ctx) : nullptr);
        if (exact) {
          // the coarse level solved exactly: block cyclic reduction over the breadth-first levels of the solid vertices, operators
          // precomputed at the Jacobian refresh (fsi_bcr.hip) - 2 log2(blocks) + 1 launches instead of sbmg_cits dependent sweeps;
          // the restriction wrote the right-hand side in the solve's own order and the prolongation reads the answer there
          FSICHK(bcr_solve(ctx, nullptr, nullptr, st));
          ctx->bcr_solves += 1;
        } else {
          const double cl = ctx->sbmg_clmax, clmin = cl / ctx->sbmg_ckappa, cth = 0.5 * (cl + clmin), cde = 0.5 * (cl - clmin), csig = cth / cde;
          double crho = 1.0 / csig;
          launch_cheb_init_b3(st, nc, crhs, ctx->sbmg_cbinv12.p, (float)(1.0 / cth), cx, cr, cd);
          HIPCHK(hipMemsetAsync(cd2, 0, n4c * sizeof(float), st));
          float *ca = cd, *cb = cd2;
          const int cits = (ctx->sbmg_cits > 0 && drop) ? ctx->sbmg_cits - 1 : ctx->sbmg_cits;
          if (cits < ctx->sbmg_cits) cx_d = ca;
          for (int k = 0; k < cits; ++k) {
            const double rn = 1.0 / (2.0 * csig - crho);
            launch_sweep_sb_b3(st, nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cbinv12.p, (float)(rn * crho),
                               (float)(2.0 * rn / cde), ca, cb, cx, cr, 1);
            std::swap(ca, cb);
            crho = rn;
            if (cx_d) cx_d = ca;
          }
        }
        launch_sbmg_prolong(st, ctx->nS, ctx->sbmg_par.p, ctx->sbmg_pw.p, ctx->sbmg_flag.p, cx, dcur,     // correction as the next direction
                            exact ? bcr_pos(ctx) : nullptr, exact ? bcr_sol(ctx) : nullptr, cx_d);
        // the restart and the post-smoothing sweeps are one chain whose last sweep is left to the scatter (with sbmg_post = 0
        // that is the restart itself: x += P x_c happens there, A P x_c is not formed)
        const int tail = drop ? ctx->sbmg_post : ctx->sbmg_post + 1;
        if (tail > 0) sweep(0.f, (float)sinit, -1);            // x += P x_c, r -= A P x_c, restart the recurrence
        srho = 1.0 / ssig;
        for (int k = 0; k + 1 < tail; ++k) {
          if (s4) { float c1, c2; s4c(k + 1, &c1, &c2); sweep(c1, c2, -1); continue; }
          const double rn = 1.0 / (2.0 * ssig - srho);
          sweep((float)(rn * srho), (float)(2.0 * rn / sde), -1);
          srho = rn;
        }
        if (drop) xs_d = dcur;
        ctx->inner_its[0] += ctx->sbmg_pre + tail;
        ctx->ss_samples_pending = (ctx->sample_budget > 0 && ctx->ss_ev0[0]) ? std::min(8, ctx->sbmg_pre) : 0;
      } else {
      const int its_s = (ctx->cheb_its_s > 0 && drop) ? ctx->cheb_its_s - 1 : ctx->cheb_its_s;
      for (int k = 0; k < its_s; ++k) {
        const bool timed = ctx->sample_budget > 0 && k < 8 && ctx->ss_ev0[0];
        const double rn = 1.0 / (2.0 * sig - rho);
        if (timed) (void)hipEventRecord(ctx->ss_ev0[k], st);
        if (fused) {
          if (ctx->sb_rec32.p)
            launch_sweep_sb_r(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_rec32.p, ctx->sb_binv12.p, (float)(rn * rho), (float)(2.0 * rn / de),
                              dcur, dnext, fx, fr);
          else
            launch_sweep_sb_b3(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, ctx->sb_binv12.p, (float)(rn * rho),
                               (float)(2.0 * rn / de), dcur, dnext, fx, fr);
          std::swap(dcur, dnext);
          if (timed) (void)hipEventRecord(ctx->ss_ev1[k], st);
        } else {
          launch_spmv_sb(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, fd, ft);
          if (timed) (void)hipEventRecord(ctx->ss_ev1[k], st);
          if (bj) launch_cheb_step_b3(st, ctx->nS, ft, ctx->sb_binv12.p, (float)(rn * rho), (float)(2.0 * rn / de), fx, fr, fd);
          else launch_cheb_step_f32(st, n, ft, ctx->sb_dinv.p, (float)(rn * rho), (float)(2.0 * rn / de), fx, fr, fd);
        }
        rho = rn;
      }
      if (its_s < ctx->cheb_its_s) xs_d = dcur;      // (unfused sweeps keep the direction in fd = dcur)
      ctx->inner_its[0] += its_s;
      ctx->ss_samples_pending = (ctx->sample_budget > 0 && ctx->ss_ev0[0]) ? std::min(8, its_s) : 0;
      }
      // xs is written by this scatter alone (the sweeps' work areas end below it): its non-solid entries stay zero from one
      // application to the next, so the 3 N2-entry fill runs once per context instead of once per application
      if (ctx->xs_zeroed != xs) { launch_fill(st, xs, n3, 0.0); ctx->xs_zeroed = xs; }
      launch_scatter3_f32(st, ctx->nS, ctx->snode.p, fx, xs, xs_d);
    } else {
    ctx->xs_zeroed = nullptr;
    ctx->inner_its[0] += ctx->cheb_its_s;
    launch_gather3(st, ctx->nS, ctx->snode.p, rv, cs_rhs);
    {
      const CsrRef M = ss_ref(ctx);
      int sample = 0;
      cheb_solve_op(ctx, M.n,
                    [&](const double* in, double* out) {
                      const bool timed = ctx->sample_budget > 0 && sample < 8 && ctx->ss_ev0[0];
                      if (timed) (void)hipEventRecord(ctx->ss_ev0[sample], st);
                      launch_spmv(st, M.n, M.rowptr, M.cols, M.vals, in, out, SPMV_SOLID_BLOCK);
                      if (timed) (void)hipEventRecord(ctx->ss_ev1[sample], st);
                      sample += timed ? 1 : 0;
                    },
                    M.vals, M.diagpos, nullptr, cs_rhs, cs_x, IW, ctx->cheb_its_s, ctx->lmax_s, ctx->cheb_kappa_s);
      ctx->ss_samples_pending = sample;
    }
    launch_fill(st, xs, n3, 0.0);
    launch_scatter3(st, ctx->nS, ctx->snode.p, cs_x, xs);
    }
    if (conc) {
      // when the solid predictor is there, the rest of the pressure step follows on B while A goes on to the displacement block
      HIPCHK(hipEventRecord(ctx->ev_solid, sA));
      HIPCHK(hipStreamWaitEvent(sB, ctx->ev_solid, 0));
      st = sB;
    } else {
    // rhs of the fluid part: rv - Avv~ xs; xs lives on the solid nodes, the fluid solve masks the solid rows, so only
    // the fluid rows with solid columns differ from rv
    launch_copy(st, rhs2, rv, n3);
    if (!ctx->vel_jacobi)      // (vel_jacobi: block Jacobi instead of Gauss-Seidel between the solid and the fluid part of the predictor)
      launch_residual_rows(st, ctx->nfs, ctx->fs_rows.p, ctx->fs_ptr.p, ctx->fs_col.p, ctx->fs_src.p, ctx->Mvv.vals.p, xs, rv, rhs2);
    }
    if (conc) {}
    else if (ctx->sweeps_fp32)
      sweeps_f = cheb_db_f32(ctx, ctx->vv_db32.p, ctx->vvf_dinv32.p, rhs2, xf, IW, ctx->cheb_its_f, ctx->lmax_f, ctx->cheb_kappa_f);
    else {
      sweeps_f = ctx->cheb_its_f;
      cheb_solve_op(ctx, n3, [&](const double* in, double* out) { launch_spmv_db(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->vv_db.p, in, out); },
                    ctx->Mvv.vals.p, ctx->diagpos3.p, ctx->mask_f.p, rhs2, xf, IW, ctx->cheb_its_f, ctx->lmax_f, ctx->cheb_kappa_f);
    }
    launch_axpby(st, vs, 1.0, xs, 1.0, xf, n3);
    ctx->inner_its[0] += sweeps_f;               // (the solid part counted its own sweeps above)
  }
  // pressure: S dp = rp - Apv~ vs,  S x = App x - Apv~ D^-1 Avp x
  if (ctx->pv32_ok)
    launch_pres_rhs32(st, V, ctx->vrank.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->rowptr_pv.p, ctx->Apv32.p,
                      (ctx->tune.experiment & 1) ? IW + 5 * n3 : vs, rp, tp);      // experiment bit 0: pressure rhs from the FLUID predictor only
  else
    launch_pres_rows(st, V, ctx->rowptr_pp.p, ctx->cols_pp.p, ctx->App.p, nullptr, 0.0, ctx->rowptr_pv.p, ctx->cols_pv.p,
                     ctx->Apv.p, vs, -1.0, rp, 1.0, tp);
  if (ctx->cheb_its_p > 0 && ctx->schur_fp32 && ctx->s_vals32.p) {
    // matrix values in FP16 / FP32, vectors in FP64 (k_sweep_schur_tiled / k_sweep_csr_mixed).  (All-FP32 vectors were measured in
    // round 2: their rounding noise exceeds the velocity residual on a coarse mesh and the outer iteration stalls.)
    const double lmax = ctx->lmax_p, lmin = lmax / ctx->cheb_kappa_p, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
    double rho = 1.0 / sig;
    {
      double *pr = conc ? rp + V : IW, *pa = pr + V, *pb = pr + 2 * V;
      // FSI_CHEB4 bit 2: the Schur sweeps as the 4th-kind polynomial (needs lmax only; see the solid block)
      const bool p4 = (ctx->cheb4 & 4) != 0;
      launch_cheb_init(st, V, nullptr, tp, ctx->s_diagpos.p, ctx->s_vals.p, p4 ? 4.0 / (3.0 * lmax) : 1.0 / th, dp, pr, pa);
      const bool tiled16 = ctx->schur_tiled && ctx->sweeps_fp16 && ctx->s_rec.p;
      const int its_p = drop ? ctx->cheb_its_p - 1 : ctx->cheb_its_p;
      for (int k = 0; k < its_p; ++k) {
        const double rn = 1.0 / (2.0 * sig - rho);
        const int i4 = k + 1;
        const double c1 = p4 ? (2.0 * i4 - 1.0) / (2.0 * i4 + 3.0) : rn * rho;
        const double c2 = p4 ? (8.0 * i4 + 4.0) / ((2.0 * i4 + 3.0) * lmax) : 2.0 * rn / de;
        const bool timed = ctx->sample_budget > 0 && k < 4 && ctx->sch_ev0[0];
        if (timed) (void)hipEventRecord(ctx->sch_ev0[k], st);
        if (tiled16)
          launch_sweep_schur_tiled(st, ctx->schur_tile, V, ctx->s_tile_max_nu, ctx->s_rowptr.p, ctx->s_rec.p, ctx->s_tile_uptr.p, ctx->s_tile_ulist.p,
                                   ctx->s_dinv.p, c1, c2, pa, pb, dp, pr);
        else
        launch_sweep_csr_mixed(st, V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals32.p, ctx->s_diagpos.p, ctx->s_vals.p, c1,
                               c2, pa, pb, dp, pr);
        if (timed) { (void)hipEventRecord(ctx->sch_ev1[k], st); ctx->sch_samples_pending = k + 1; }
        std::swap(pa, pb);
        rho = rn;
      }
      // the dropped last sweep's x += d: V doubles, a launch of its own in front of the velocity correction
      if (its_p < ctx->cheb_its_p) launch_axpby(st, dp, 1.0, dp, 1.0, pa, V);
      ctx->inner_its[1] += its_p;
    }
  } else if (ctx->cheb_its_p > 0 && ctx->fused_sweeps) {
    // all-FP64 Schur sweeps, product fused with the Chebyshev update (one launch per sweep)
    const double lmax = ctx->lmax_p, lmin = lmax / ctx->cheb_kappa_p, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
    double rho = 1.0 / sig;
    double *pr = conc ? rp + V : IW, *pa = pr + V, *pb = pr + 2 * V;      // two chains: the Schur vectors live in the unused tail of rp, IW is stream A's
    launch_cheb_init(st, V, nullptr, tp, ctx->s_diagpos.p, ctx->s_vals.p, 1.0 / th, dp, pr, pa);
    const int its_p = drop ? ctx->cheb_its_p - 1 : ctx->cheb_its_p;
    for (int k = 0; k < its_p; ++k) {
      const double rn = 1.0 / (2.0 * sig - rho);
      const bool timed = ctx->sample_budget > 0 && k < 4 && ctx->sch_ev0[0];
      if (timed) (void)hipEventRecord(ctx->sch_ev0[k], st);
      if (ctx->schur_tiled)      // the tiles of the FP16 form with the FP64 values: bitwise the sweep of launch_sweep_csr_f64
        launch_sweep_schur_tiled_f64(st, ctx->schur_tile, V, ctx->s_tile_max_nu, ctx->s_rowptr.p, ctx->s_vals.p, ctx->s_ploc.p,
                                     ctx->s_tile_uptr.p, ctx->s_tile_ulist.p, ctx->s_diagpos.p, rn * rho, 2.0 * rn / de, pa, pb, dp, pr);
      else
        launch_sweep_csr_f64(st, V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals.p, ctx->s_diagpos.p, rn * rho, 2.0 * rn / de, pa, pb, dp, pr);
      if (timed) { (void)hipEventRecord(ctx->sch_ev1[k], st); ctx->sch_samples_pending = k + 1; }
      std::swap(pa, pb);
      rho = rn;
    }
    if (its_p < ctx->cheb_its_p) launch_axpby(st, dp, 1.0, dp, 1.0, pa, V);      // the dropped last sweep's x += d (see above)
    ctx->inner_its[1] += its_p;
  } else if (ctx->cheb_its_p > 0) {
    int sample = 0;
    cheb_solve_op(ctx, V,
                  [&](const double* in, double* out) {
                    const bool timed = ctx->sample_budget > 0 && sample < 4 && ctx->sch_ev0[0];
                    if (timed) (void)hipEventRecord(ctx->sch_ev0[sample], st);
                    schur_apply(ctx, in, out, w3);
                    if (timed) { (void)hipEventRecord(ctx->sch_ev1[sample], st); sample += 1; ctx->sch_samples_pending = sample; }
                  },
                  ctx->s_vals.p, ctx->s_diagpos.p, nullptr, tp, dp, IW, ctx->cheb_its_p, ctx->lmax_p, ctx->cheb_kappa_p);
    ctx->inner_its[1] += ctx->cheb_its_p;
  }
  // velocity correction and displacement
  if (ctx->pv32_ok)
    launch_vel_correct32(st, N2, ctx->padj_ptr.p, ctx->padj.p, ctx->Avp32.p, dp, ctx->vv_dinv.p, vs, dv);
  else
    launch_vel_correct(st, n3, ctx->rowptr_vp.p, ctx->cols_vp.p, ctx->Avp.p, dp, ctx->diagpos3.p, ctx->Mvv.vals.p, vs, dv, ctx->vv_dinv.p);
  if (conc) { HIPCHK(hipEventRecord(ctx->ev_b, sB)); st = sA; }      // the rest (displacement block) is stream A's, behind the solid predictor
  if (ctx->adv_is_db) {
    // dd_early: the displacement block sees the solid PREDICTOR instead of the corrected velocity - what it has when its chain
    // runs beside the pressure step instead of after it
    // r_d - A_dv dv in place in r_d (nothing else reads it after the split): A_dv has entries in the rows of solid nodes only
    // (adv_solid_only: verified at every refresh)
    const double* vsrc = (ctx->dd_early || conc) ? IW + 4 * n3 : dv;
    if (ctx->tune.experiment & 2) {}      // (experiment bit 1: displacement block without any velocity coupling)
    else if (ctx->adv_solid_only)
      launch_db_rows_sub(st, ctx->nS, ctx->snode.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->adv_db.p, ctx->adv_rowmask.p, vsrc, rd);
    else {
      launch_spmv_db(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->adv_db.p, vsrc, w3, ctx->adv_rowmask.p);
      launch_axpby(st, rd, 1.0, rd, -1.0, w3, n3);
    }
    td = rd;
  } else {
    launch_residual_csr(st, n3, ctx->rowptr3.p, ctx->cols3.p, ctx->Adv.p, dv, rd, td);
  }
  const float *dd_f32 = nullptr, *dd_d = nullptr;      // dd_d: the displacement chain's direction, added by the merge (dropped last sweep)
  if (ctx->cheb_its_d > 0) {
    if (ctx->dd_is_scalar && ctx->sweeps_fp32) {
      // Jacobi-scaled system  (D^-1 A_dd) dd = D^-1 td  with the one-number-per-node-pair operator
      const int64_t n = 4 * N2;
      float* F = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(IW) + 15) & ~uintptr_t(15));   // float4 loads
      float *fr = F, *fd = F + n, *ft = F + 2 * n, *fx = F + 3 * n, *frhs = F + 4 * n;
      (void)frhs;
      const double lmax = ctx->lmax_d, lmin = lmax / ctx->cheb_kappa_d, th = 0.5 * (lmax + lmin), de = 0.5 * (lmax - lmin), sig = th / de;
      double rho = 1.0 / sig;
      const bool fused = ctx->tiled && ctx->fused_sweeps;
      float *dcur = fd, *dnext = ft;               // fused sweeps ping-pong the direction; ft is otherwise the product (dcur stays fd)
      const float* cx_d = nullptr;                 // the coarse chain's direction for the prolongation, when its last sweep is dropped
      auto fine_spmv = [&](int k_sample) {
        const bool timed = ctx->sample_budget > 0 && k_sample >= 0 && k_sample < 4 && ctx->sc_ev0[0];
        if (timed) (void)hipEventRecord(ctx->sc_ev0[k_sample], st);
        if (ctx->tiled)
          launch_spmv_tiled_f32(st, 1, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_chat.p, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                                ctx->dd_rowflag.p, fd, ft);
        else
          launch_spmv_sc_f32(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_chat.p, ctx->dd_rowflag.p, fd, ft);
        if (timed) { (void)hipEventRecord(ctx->sc_ev1[k_sample], st); ctx->sc_samples_pending = k_sample + 1; }
      };
      // one sweep: product + Chebyshev update (one launch when fused)
      auto fine_sweep = [&](float c1, float c2, int k_sample) {
        if (!fused) {
          fine_spmv(k_sample);
          launch_cheb_step_f32(st, n, ft, ctx->ones32.p, c1, c2, fx, fr, fd);
          return;
        }
        const bool timed = ctx->sample_budget > 0 && k_sample >= 0 && k_sample < 4 && ctx->sc_ev0[0];
        if (timed) (void)hipEventRecord(ctx->sc_ev0[k_sample], st);
        if (ctx->sweeps_fp16)
          launch_sweep_tiled_h(st, 1, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_rec.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                               ctx->dd_rowflag.p, nullptr, c1, c2, dcur, dnext, fx, fr);
        else      // k_sweep_tiled_f32<1> with two rows ahead in flight (same arrays, same sums)
          launch_sweep_tiled_a1(st, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_chat.p, ctx->tile_ploc.p, ctx->tile_uptr.p,
                                ctx->tile_ulist.p, ctx->dd_rowflag.p, nullptr, c1, c2, dcur, dnext, fx, fr);
        if (timed) { (void)hipEventRecord(ctx->sc_ev1[k_sample], st); ctx->sc_samples_pending = k_sample + 1; }
        std::swap(dcur, dnext);
      };
      if (ctx->mg_ready) {
        // two-level cycle: Chebyshev smoothing on [lmax/alpha, lmax], coarse solve on the vertex graph, smoothing again
        const double slmin = lmax / ctx->mg_alpha, sth = 0.5 * (lmax + slmin), sde = 0.5 * (lmax - slmin), ssig = sth / sde;
        double srho = 1.0 / ssig;
        const bool d4 = (ctx->cheb4 & 2) != 0;                 // FSI_CHEB4 bit 1: 4th-kind smoothing sweeps (see the solid block)
        const double dinit = d4 ? 4.0 / (3.0 * lmax) : 1.0 / sth;
        auto d4c = [&](int i, float* c1, float* c2) { *c1 = (float)((2.0 * i - 1.0) / (2.0 * i + 3.0)); *c2 = (float)((8.0 * i + 4.0) / ((2.0 * i + 3.0) * lmax)); };
        launch_pad_init_f32(st, N2, td, ctx->dd_dinv32.p, ctx->ones32.p, (float)dinit, fx, fr, fd);      // Jacobi scaling + initialise
        for (int k = 0; k < ctx->mg_pre; ++k) {
          if (d4) { float c1, c2; d4c(k + 1, &c1, &c2); fine_sweep(c1, c2, k); continue; }
          const double rn = 1.0 / (2.0 * ssig - srho);
          fine_sweep((float)(rn * srho), (float)(2.0 * rn / sde), k);
          srho = rn;
        }
        const int64_t nc = ctx->mg_nc, n4c = 4 * nc;
        float *cr = ctx->mg_work.p, *cd = cr + n4c, *ct = cr + 2 * n4c, *cx = cr + 3 * n4c, *crhs = cr + 4 * n4c;
        {
          const double cl = ctx->mg_clmax, clmin = cl / ctx->mg_ckappa, cth = 0.5 * (cl + clmin), cde = 0.5 * (cl - clmin), csig = cth / cde;
          double crho = 1.0 / csig;
          // restriction and the coarse recurrence's start (x = 0, r = rhs, d = rhs / theta) in one launch
          launch_mg_restrict(st, nc, ctx->mg_chptr.p, ctx->mg_child.p, ctx->mg_chw.p, ctx->mg_d0.p, fr, ctx->mg_dcinv4.p, crhs,
                             (float)(1.0 / cth), cx, cr, cd);
          (void)n4c;
          float *ca = cd, *cb = ct;
          const int cits = (ctx->mg_cits > 0 && drop) ? ctx->mg_cits - 1 : ctx->mg_cits;
          for (int k = 0; k < cits; ++k) {
            const double rn = 1.0 / (2.0 * csig - crho);
            if (ctx->fused_sweeps) {
              launch_sweep_sc_f32(st, nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, (float)(rn * crho),
                                  (float)(2.0 * rn / cde), ca, cb, cx, cr);
              std::swap(ca, cb);
            } else {
              launch_spmv_sc_f32(st, nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, cd, ct);
              launch_cheb_step_f32(st, n4c, ct, ctx->mg_cones.p, (float)(rn * crho), (float)(2.0 * rn / cde), cx, cr, cd);
            }
            crho = rn;
          }
          if (cits < ctx->mg_cits) cx_d = ca;      // (unfused coarse sweeps keep the direction in cd = ca)
        }
        launch_mg_prolong(st, N2, ctx->mg_par.p, ctx->mg_pw.p, ctx->mg_d0.p, cx, dcur, cx_d);   // correction as the next direction
        // restart + post-smoothing: one chain, its last sweep left to the merge (with mg_post = 0 the restart itself, see the solid cycle)
        const int tail = drop ? ctx->mg_post : ctx->mg_post + 1;
        if (tail > 0) fine_sweep(0.f, (float)dinit, -1);                               // x += P x_c, r -= C P x_c, restart
        srho = 1.0 / ssig;
        for (int k = 0; k + 1 < tail; ++k) {
          if (d4) { float c1, c2; d4c(k + 1, &c1, &c2); fine_sweep(c1, c2, -1); continue; }
          const double rn = 1.0 / (2.0 * ssig - srho);
          fine_sweep((float)(rn * srho), (float)(2.0 * rn / sde), -1);
          srho = rn;
        }
        if (drop) dd_d = dcur;
        ctx->inner_its[2] += ctx->mg_pre + tail;
      } else {
        launch_pad_init_f32(st, N2, td, ctx->dd_dinv32.p, ctx->ones32.p, (float)(1.0 / th), fx, fr, fd);
        const int its_d = drop ? ctx->cheb_its_d - 1 : ctx->cheb_its_d;
        for (int k = 0; k < its_d; ++k) {
          const double rn = 1.0 / (2.0 * sig - rho);
          fine_sweep((float)(rn * rho), (float)(2.0 * rn / de), k);
          rho = rn;
        }
        if (its_d < ctx->cheb_its_d) dd_d = dcur;
        ctx->inner_its[2] += its_d;
      }
      dd_f32 = fx;                                  // the merge below takes the displacement part straight from the sweeps' result
      if (ctx->debug_prec_apply > 0) launch_unpad_from_f32(st, N2, fx, dd, dd_d);
    } else if (ctx->dd_is_db && ctx->sweeps_fp32)
      ctx->inner_its[2] += cheb_db_f32(ctx, ctx->dd_db32.p, ctx->dd_dinv32.p, td, dd, IW, ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d);
    else if (ctx->dd_is_db) {
      ctx->inner_its[2] += ctx->cheb_its_d;
      cheb_solve_op(ctx, n3, [&](const double* in, double* out) { launch_spmv_db(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p, in, out); },
                    ctx->Mdd.vals.p, ctx->diagpos3.p, nullptr, td, dd, IW, ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d);
    } else {
      ctx->inner_its[2] += ctx->cheb_its_d;
      cheb_solve(ctx, CsrRef{n3, ctx->rowptr3.p, ctx->cols3.p, ctx->Mdd.vals.p, ctx->diagpos3.p}, nullptr, td, dd, IW,
                 ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d);
    }
  }
  if (conc) HIPCHK(hipStreamWaitEvent(sA, ctx->ev_b, 0));
  if (dd_f32) launch_merge_f32d(st, N2, V, dd_f32, dv, dp, z, dd_d);
  else launch_merge(st, N2, V, dd, dv, dp, z);
  if (ctx->debug_prec_apply > 0) {                 // FSI_DEBUG_PRECOND=2: non-finite entries of the parts, first applications only
    ctx->debug_prec_apply -= 1;
    auto bad = [&](const double* p, int64_t n) { std::vector<double> h(n); (void)hipMemcpy(h.data(), p, n * sizeof(double), hipMemcpyDeviceToHost);
                                                  int64_t b = 0; double m = 0.0; for (double v : h) { if (!std::isfinite(v)) b++; else m = std::max(m, std::fabs(v)); }
                                                  return std::make_pair(b, m); };
    const auto bt = bad(tp, V), bp = bad(dp, V), bv = bad(dv, n3), bd = bad(dd, n3), bs = bad(vs, n3);
    fprintf(stderr, "[precond] apply: rhs_p max %.3e (%lld bad)  dp max %.3e (%lld bad)  v* max %.3e (%lld bad)  dv max %.3e (%lld bad)  dd max %.3e (%lld bad)\n",
            bt.second, (long long)bt.first, bp.second, (long long)bp.first, bs.second, (long long)bs.first, bv.second, (long long)bv.first, bd.second, (long long)bd.first);
  }
  ctx->inner_calls += 1;
  if (ctx->sample_budget > 0) ctx->sample_budget -= 1;
  if (ctx->sc_samples_pending > 0) {      // sampled launch durations of the scalar-ratio displacement SpMV
    (void)hipEventSynchronize(ctx->sc_ev1[ctx->sc_samples_pending - 1]);
    for (int k = 0; k < ctx->sc_samples_pending; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->sc_ev0[k], ctx->sc_ev1[k]) == hipSuccess) { ctx->t_sc.ms += ms; ctx->t_sc.calls += 1; }
    }
    ctx->sc_samples_pending = 0;
  }
  if (ctx->sch_samples_pending > 0) {     // sampled launch durations of the Schur-complement sweeps
    (void)hipEventSynchronize(ctx->sch_ev1[ctx->sch_samples_pending - 1]);
    for (int k = 0; k < ctx->sch_samples_pending; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->sch_ev0[k], ctx->sch_ev1[k]) == hipSuccess) { ctx->t_sch.ms += ms; ctx->t_sch.calls += 1; }
    }
    ctx->sch_samples_pending = 0;
  }
  if (ctx->db_samples_pending > 0) {      // sampled launch durations of the FP32 component-diagonal SpMV
    (void)hipEventSynchronize(ctx->db_ev1[ctx->db_samples_pending - 1]);
    for (int k = 0; k < ctx->db_samples_pending; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->db_ev0[k], ctx->db_ev1[k]) == hipSuccess) { ctx->t_db.ms += ms; ctx->t_db.calls += 1; }
    }
    ctx->db_samples_pending = 0;
  }
  if (ctx->ss_samples_pending > 0) {      // sampled launch durations of the solid-block SpMV (first 8 of every apply)
    (void)hipEventSynchronize(ctx->ss_ev1[ctx->ss_samples_pending - 1]);
    for (int k = 0; k < ctx->ss_samples_pending; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->ss_ev0[k], ctx->ss_ev1[k]) == hipSuccess) { ctx->t_ss.ms += ms; ctx->t_ss.calls += 1; }
    }
    ctx->ss_samples_pending = 0;
  }
  return FSI_OK;
}

int precondition(FsiCtx* ctx, const double* r, double* z) {
  Phase ph(ctx, &ctx->t_prec);
  if (ctx->precond == 0) return precondition_block(ctx, r, z);
  launch_sptrsv_levels(ctx->stream, ctx->levels, ctx->rowptr.p, ctx->cols.p, ctx->diagpos.p, ctx->LU.p, r, ctx->tmp7.p, z);
  return FSI_OK;
}
}  // namespace host
}  // namespace fsi

// Factorisations for the active preconditioner, from the row-equilibrated Jacobian in ctx->A.
namespace {
// Largest eigenvalue of a coarse level's scaled operator by power iteration with the level's own sweep kernel: a sweep with
// c1 = 0, c2 = 1 on a zero residual returns d_out = -(scaled operator) d_in.  The Gershgorin row-sum bound the levels used
// in round 2 is 2.2x the true value on the solid vertices of the bench mesh - every Chebyshev interval [bound / kappa, bound]
// built on it reaches that much less far down the spectrum for the same number of sweeps.  work: 4 vectors of n4 floats.
template <class Sweep>
int coarse_power_lmax(FsiCtx* ctx, int64_t nnodes, float* work, Sweep&& sweep, double bound, double* out) {
  hipStream_t st = ctx->stream;
  const int64_t n4 = 4 * nnodes;
  float *r = work, *da = work + n4, *db = work + 2 * n4, *x = work + 3 * n4;
  launch_f32_ripple4(st, nnodes, da);
  double* acc = ctx->scratch.p + 4100;
  const int its = 30;
  for (int k = 0; k < its; ++k) {
    HIPCHK(hipMemsetAsync(r, 0, n4 * sizeof(float), st));
    sweep(da, db, x, r);
    std::swap(da, db);
    if (k == its - 2) launch_f32_sumsq(st, n4, da, acc);
    if (k == its - 1) launch_f32_sumsq(st, n4, da, acc + 1);
  }
  double h[2] = {0.0, 0.0};
  HIPCHK(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *out = bound;
  if (h[0] > 0.0 && h[1] > 0.0 && std::isfinite(h[0]) && std::isfinite(h[1])) {
    const double lam = std::sqrt(h[1] / h[0]);
    if (std::isfinite(lam) && lam > 0.0) *out = std::min(bound, 1.2 * lam);      // same head room as the fine levels' estimates
  }
  return FSI_OK;
}
}  // namespace

namespace fsi {
namespace host {

int refresh_preconditioner(FsiCtx* ctx) {
  Phase ph(ctx, &ctx->t_fac);
  ctx->xs_zeroed = nullptr;          // (the refresh uses ctx->blk as scratch: the next application zeroes its solid-predictor vector again)
  hipStream_t st = ctx->stream;
  int32_t flags[4] = {0, 0, 0, 0};
  if (!ctx->coloured && ctx->precond != 0) {
    ctx->err = "the monolithic ILU(0) preconditioner needs the multicolour node ordering: create the context with FSI_ORDER=colour";
    return FSI_ERR_INVALID;
  }
  if (ctx->precond == 0) {
    launch_extract_blocks(st, ctx->N2, ctx->V, ctx->scheme.k * ctx->scheme.th0, ctx->rowptr.p, ctx->A.p, ctx->nadj_ptr.p,
                          ctx->nadj.p, ctx->padj_ptr.p, ctx->vrank.p, ctx->node_solid.p, ctx->rowptr3.p, ctx->rowptr_vp.p,
                          ctx->rowptr_pv.p, ctx->rowptr_pp.p, ctx->Mdd.vals.p, ctx->Adv.p, ctx->Mvv.vals.p, ctx->Avp.p,
                          ctx->Apv.p, ctx->App.p);
    HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
    launch_schur_full(st, ctx->V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->vrank.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->padj_ptr.p,
                      ctx->padj.p, ctx->rowptr_pv.p, ctx->Apv.p, ctx->rowptr_pp.p, ctx->App.p, ctx->rowptr_vp.p, ctx->Avp.p,
                      ctx->diagpos3.p, ctx->Mvv.vals.p, ctx->s_vals.p, ctx->iflags.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
    if (flags[1] & 4) { ctx->err = "Schur complement: a vertex has too many (two-ring) vertex neighbours"; return FSI_ERR_INVALID; }
    {
      const int64_t npairs = (int64_t)ctx->dd_db.n / 3;
      launch_extract_db(st, ctx->N2, npairs, ctx->nadj_ptr.p, ctx->rowptr3.p, ctx->Mdd.vals.p, ctx->dd_db.p, ctx->iflags.p, 1);
      launch_extract_db(st, ctx->N2, npairs, ctx->nadj_ptr.p, ctx->rowptr3.p, ctx->Mvv.vals.p, ctx->vv_db.p, ctx->iflags.p, 0);
      HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
      ctx->dd_is_db = !(flags[1] & 8);      // A_dd acts per component (always so for the forms of SURVEY.md A.2)
      HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      launch_extract_db(st, ctx->N2, npairs, ctx->nadj_ptr.p, ctx->rowptr3.p, ctx->Adv.p, ctx->adv_db.p, ctx->iflags.p, 1);
      HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
      ctx->adv_is_db = !(flags[1] & 8);
      ctx->pv32_ok = false;
      if (ctx->tune.pv_fp32) {      // FP32 copies for the two block products of the pressure step
        if (!ctx->Avp32.p) { HIPCHK(ctx->Avp32.alloc(ctx->Avp.n)); HIPCHK(ctx->Apv32.alloc(ctx->Apv.n)); }
        launch_to_f32(st, (int64_t)ctx->Avp.n, ctx->Avp.p, ctx->Avp32.p);
        launch_to_f32(st, (int64_t)ctx->Apv.n, ctx->Apv.p, ctx->Apv32.p);
        ctx->pv32_ok = true;
      }
      if (!ctx->vv_dinv.p) HIPCHK(ctx->vv_dinv.alloc(3 * ctx->N2));
      launch_diag_inverse(st, 3 * ctx->N2, ctx->diagpos3.p, ctx->Mvv.vals.p, ctx->vv_dinv.p);
      if (!ctx->adv_rowmask.p) HIPCHK(ctx->adv_rowmask.alloc(ctx->N2));
      launch_db_rowmask(st, ctx->N2, ctx->nadj_ptr.p, ctx->adv_db.p, ctx->adv_rowmask.p);     // A_dv has no entries in fluid rows
      HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      launch_mask_outside(st, ctx->N2, ctx->adv_rowmask.p, ctx->node_solid.p, ctx->iflags.p);      // ... checked, not assumed
      HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
      ctx->adv_solid_only = flags[0] == 0;
      HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      launch_extract_chat(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p, ctx->dd_chat.p, ctx->dd_rowflag.p, ctx->iflags.p);
      HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
      ctx->dd_is_scalar = ctx->dd_is_db && !(flags[1] & 16) && ctx->tune.scalar_dd;
      // The displacement block (solid mass + mesh Laplacian with a constant coefficient) does not change from one Jacobian
      // to the next for the forms VaSP uses: what is derived from it alone - its coarse operator here, its eigenvalue
      // estimate below - is kept while a checksum of the block's values (sum of squares, one pass) stays the same.
      // Three numbers: the sum of squares, a sum with index-hashed weights (sign changes, permuted entries, entries
      // far below the largest one) and the same hashed sum over the row scaling of the d rows, which the Galerkin product
      // takes as a separate input.  fsi_get_timers counts the hits (dd_cache_hits).
      double cs[3] = {0.0, 0.0, 0.0};
      FSICHK(dot_n(ctx, ctx->Mdd.vals.p, ctx->Mdd.vals.p, (int64_t)ctx->Mdd.nnz, &cs[0]));
      launch_hashed_sum(st, ctx->Mdd.vals.p, 0, 1, (int64_t)ctx->Mdd.nnz, ctx->scratch.p, ctx->scratch.p + 4096);
      FSICHK(host_scalar(ctx, ctx->scratch.p + 4096, &cs[1]));
      for (int c = 0; c < 3; ++c) {
        double part = 0.0;
        launch_hashed_sum(st, ctx->rowscale.p, c, 6, ctx->N2, ctx->scratch.p, ctx->scratch.p + 4096);
        FSICHK(host_scalar(ctx, ctx->scratch.p + 4096, &part));
        cs[2] += (c + 1) * part;
      }
      bool same = ctx->dd_checksum_valid;
      for (int k = 0; k < 3; ++k) same = same && std::isfinite(cs[k]) && std::fabs(cs[k] - ctx->dd_checksum[k]) <= 1e-12 * std::fabs(cs[k]);
      ctx->dd_same = same;
      for (int k = 0; k < 3; ++k) ctx->dd_checksum[k] = cs[k];
      ctx->dd_checksum_valid = std::isfinite(cs[0]) && std::isfinite(cs[1]) && std::isfinite(cs[2]);
      if (ctx->dd_same) ctx->dd_cache_hits += 1;
      const bool mg_keep_on = ctx->tune.mg_keep != 0;
      const bool mg_keep = mg_keep_on && ctx->dd_same && ctx->mg_ready && ctx->dd_mg && ctx->dd_is_scalar && ctx->sweeps_fp32 && ctx->mg_nc > 0;
      if (!mg_keep) ctx->mg_ready = false;
      if (!mg_keep && ctx->dd_mg && ctx->dd_is_scalar && ctx->sweeps_fp32 && ctx->mg_nc > 0) {
        // Galerkin coarse operator of the displacement block, A_c = P^T A0 P, and its Jacobi-scaled single-precision form
        HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
        HIPCHK(hipMemsetAsync(ctx->mg_Ac.p, 0, ctx->mg_cnnz * sizeof(double), st));
        launch_mg_d0(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p, ctx->rowscale.p, ctx->dd_rowflag.p, ctx->mg_d0.p, ctx->iflags.p);
        launch_mg_rap(st, ctx->mg_nc, ctx->mg_chptr.p, ctx->mg_child.p, ctx->mg_chw.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p,
                      ctx->rowscale.p, ctx->dd_rowflag.p, ctx->mg_par.p, ctx->mg_pw.p, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_Ac.p,
                      ctx->iflags.p);
        launch_mg_coarse_finish(st, ctx->mg_nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_Ac.p, ctx->mg_cfine.p, ctx->dd_rowflag.p,
                                ctx->mg_cc.p, ctx->mg_cflag.p, ctx->mg_dcinv4.p, ctx->iflags.p + 2);
        HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
        float rowmax;
        std::memcpy(&rowmax, &flags[2], sizeof rowmax);
        ctx->mg_ready = !(flags[1] & (32 | 64)) && std::isfinite(rowmax) && rowmax > 0.f;
        ctx->mg_clmax = ctx->mg_gersh = rowmax;   // Gershgorin bound of the Jacobi-scaled coarse operator
        if (ctx->mg_ready && ctx->coarse_power) {
          double lam = rowmax;
          FSICHK(coarse_power_lmax(ctx, ctx->mg_nc, ctx->mg_work.p,
                                   [&](const float* din, float* dout, float* x, float* r) {
                                     launch_sweep_sc_f32(st, ctx->mg_nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, 0.f, 1.f, din, dout, x, r);
                                   }, rowmax, &lam));
          if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] displacement coarse level: lmax %.3f by power iteration (Gershgorin bound %.3f)\n", lam, (double)rowmax);
          ctx->mg_clmax = lam;
        }
        HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      }
      launch_to_f32(st, 3 * npairs, ctx->dd_db.p, ctx->dd_db32.p);
      launch_to_f32(st, 3 * npairs, ctx->vv_db.p, ctx->vv_db32.p);
      if (ctx->sweeps_fp16 && ctx->tiled) {      // packed FP16 records of the two tiled operators (see k_pack_h1 / k_pack_h3)
        if (!ctx->dd_rec.p) { HIPCHK(ctx->dd_rec.alloc(npairs)); HIPCHK(ctx->vv_rec.alloc(2 * npairs)); }
        launch_pack_h1(st, npairs, ctx->dd_chat.p, ctx->tile_ploc.p, ctx->dd_rec.p);
        launch_pack_h3(st, npairs, ctx->vv_db32.p, ctx->tile_ploc.p, ctx->vv_rec.p);
      } else if (ctx->tiled && ctx->fused_sweeps && ctx->sweeps_fp32) {   // FP32 records of the fluid block (k_pack_f3): three values and the index in one load
        if (!ctx->vv_rec32.p) HIPCHK(ctx->vv_rec32.alloc(4 * npairs));
        launch_pack_f3(st, npairs, ctx->vv_db32.p, ctx->tile_ploc.p, ctx->vv_rec32.p);
      }
      launch_dinv_f32(st, ctx->N2, nullptr, ctx->diagpos3.p, ctx->Mdd.vals.p, ctx->dd_dinv32.p);
      launch_dinv_f32(st, ctx->N2, ctx->mask_f.p, ctx->diagpos3.p, ctx->Mvv.vals.p, ctx->vvf_dinv32.p);
    }
    launch_gather_vals(st, (int64_t)ctx->ss_vals.n, ctx->ss_src.p, ctx->Mvv.vals.p, ctx->ss_vals.p);
    launch_sb_gather(st, ctx->sb_nblocks, ctx->sb_row.p, ctx->sb_src.p, ctx->sb_stride.p, ctx->Mvv.vals.p, ctx->sb_vals.p);
    if (ctx->sweeps_fp16 && ctx->solid_fp32 && ctx->sb_nblocks > 0) {
      if (!ctx->sb_rec.p) HIPCHK(ctx->sb_rec.alloc(6 * ctx->sb_nblocks));
      launch_pack_sb(st, ctx->sb_nblocks, ctx->sb_vals.p, ctx->sb_col.p, ctx->sb_rec.p);
    } else if (ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused && ctx->sb_nblocks > 0) {      // FP32 records: a block and its column in 40 bytes (k_pack_sb_f32)
      if (!ctx->sb_rec32.p) HIPCHK(ctx->sb_rec32.alloc(10 * ctx->sb_nblocks));
      launch_pack_sb_f32(st, ctx->sb_nblocks, ctx->sb_vals.p, ctx->sb_col.p, ctx->sb_rec32.p);
    }
    launch_sb_dinv(st, ctx->nS, ctx->snode.p, ctx->diagpos3.p, ctx->Mvv.vals.p, ctx->sb_dinv.p);
    launch_sb_binv(st, ctx->nS, ctx->snode.p, ctx->diagpos3.p, ctx->Mvv.vals.p, ctx->sb_binv12.p, ctx->sb_binv9.p);
    ctx->sbmg_ready = false;
    if (ctx->solid_mg && ctx->sbmg_nc > 0 && ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused) {
      HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      HIPCHK(hipMemsetAsync(ctx->sbmg_cvals.p, 0, 9 * ctx->sbmg_nblk * sizeof(float), st));
      launch_sbmg_flags(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, ctx->sbmg_flag.p);
      launch_sbmg_rap(st, ctx->sbmg_nc, ctx->sbmg_chptr.p, ctx->sbmg_child.p, ctx->sbmg_chw.p, ctx->sb_ptr.p, ctx->sb_col.p,
                      ctx->sb_vals.p, ctx->snode.p, ctx->rowscale.p, ctx->sbmg_flag.p, ctx->sbmg_par.p, ctx->sbmg_pw.p,
                      ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->iflags.p);
      launch_sbmg_coarse_finish(st, ctx->sbmg_nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cfine.p,
                                ctx->sbmg_flag.p, ctx->sbmg_cbinv12.p, ctx->sbmg_cflag.p, ctx->iflags.p + 2);
      HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
      float rowmax;
      std::memcpy(&rowmax, &flags[2], sizeof rowmax);
      ctx->sbmg_ready = !(flags[1] & 64) && std::isfinite(rowmax) && rowmax > 0.f;
      ctx->sbmg_clmax = ctx->sbmg_gersh = rowmax;
      if (ctx->sbmg_ready && ctx->bcr && ctx->solid_coarse_exact) FSICHK(bcr_refresh(ctx));      // exact coarse solve: operators of the new matrix
      if (ctx->sbmg_ready && ctx->coarse_power && !bcr_ready(ctx)) {
        double lam = rowmax;
        FSICHK(coarse_power_lmax(ctx, ctx->sbmg_nc, ctx->sbmg_work.p,
                                 [&](const float* din, float* dout, float* x, float* r) {
                                   launch_sweep_sb_b3(st, ctx->sbmg_nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cbinv12.p, 0.f, 1.f, din, dout, x, r, 1);
                                 }, rowmax, &lam));
        if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] solid coarse level: lmax %.3f by power iteration (Gershgorin bound %.3f)\n", lam, (double)rowmax);
        ctx->sbmg_clmax = lam;
      }
      HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
      if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] solid two-level: %lld coarse nodes, clmax %.3f, ready %d\n", (long long)ctx->sbmg_nc, rowmax, (int)ctx->sbmg_ready);
    }
    if (ctx->solid_block_jacobi && ctx->solid_fp32) {      // largest eigenvalue of D_b^-1 A_SS (power iteration, as power_lmax_op)
      const CsrRef M = ss_ref(ctx);
      double *x = ctx->blk.p, *y = ctx->blk.p + M.n, lam = 1.0;
      launch_mask_ripple(st, M.n, nullptr, x);
      for (int k = 0; k < 40; ++k) {
        launch_spmv(st, M.n, M.rowptr, M.cols, M.vals, x, y, SPMV_SOLID_BLOCK);
        launch_block_scale_d(st, ctx->nS, ctx->sb_binv9.p, y);
        double xx = 0.0, yy = 0.0;
        FSICHK(dot_n(ctx, x, x, M.n, &xx));
        FSICHK(dot_n(ctx, y, y, M.n, &yy));
        if (!(xx > 0.0) || !(yy > 0.0) || !std::isfinite(yy)) break;
        lam = std::sqrt(yy / xx);
        launch_copy(st, x, y, M.n);
        launch_scale(st, x, 1.0 / std::sqrt(yy), M.n);
      }
      ctx->lmax_s = 1.2 * lam;
    } else {
      FSICHK(power_lmax(ctx, ss_ref(ctx), nullptr, ctx->blk.p, &ctx->lmax_s));
    }
    FSICHK(power_lmax_op(ctx, 3 * ctx->N2, [&](const double* in, double* o) { launch_spmv_db(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->vv_db.p, in, o); },
                         ctx->Mvv.vals.p, ctx->diagpos3.p, ctx->mask_f.p, ctx->blk.p, &ctx->lmax_f));
    {
      // its 40 power iterations on a 3 N2-row CSR matrix were 60 ms of every refresh: kept while the block is unchanged (dd_same)
      if (ctx->lmax_d_cached > 0.0 && ctx->dd_same) {
        ctx->lmax_d = ctx->lmax_d_cached;
      } else {
        FSICHK(power_lmax(ctx, CsrRef{3 * ctx->N2, ctx->rowptr3.p, ctx->cols3.p, ctx->Mdd.vals.p, ctx->diagpos3.p}, nullptr,
                          ctx->blk.p, &ctx->lmax_d));
        ctx->lmax_d_cached = ctx->lmax_d;
      }
    }
    FSICHK(power_lmax_op(ctx, ctx->V, [&](const double* in, double* o) { schur_apply(ctx, in, o, ctx->blk.p + 19 * 3 * ctx->N2); },
                         ctx->s_vals.p, ctx->s_diagpos.p, nullptr, ctx->blk.p, &ctx->lmax_p));
    if (ctx->schur_fp32) {
      if (!ctx->s_vals32.p) {
        HIPCHK(ctx->s_vals32.alloc(ctx->s_vals.n));
      }
      launch_to_f32(st, (int64_t)ctx->s_vals.n, ctx->s_vals.p, ctx->s_vals32.p);
      if (ctx->schur_tiled && ctx->sweeps_fp16) {
        if (!ctx->s_rec.p) { HIPCHK(ctx->s_rec.alloc(ctx->s_vals.n)); HIPCHK(ctx->s_dinv.alloc(ctx->V)); }
        launch_pack_h1(st, (int64_t)ctx->s_vals.n, ctx->s_vals32.p, ctx->s_ploc.p, ctx->s_rec.p);
        launch_diag_inverse(st, ctx->V, ctx->s_diagpos.p, ctx->s_vals.p, ctx->s_dinv.p);
      }
    }
    // self-test: a Chebyshev interval that misses the top of a spectrum (non-normal blocks at rough states) blows up;
    // widen the intervals until one application to a rippled vector stays finite and bounded
    ctx->prec_bad = false;
    double prev_out = 0.0;
    const double l0[4] = {ctx->lmax_s, ctx->lmax_f, ctx->lmax_p, ctx->lmax_d};
    for (int attempt = 0; attempt < 8; ++attempt) {
      launch_mask_ripple(st, ctx->ndof, nullptr, ctx->tmp1.p);
      FSICHK(precondition_block(ctx, ctx->tmp1.p, ctx->tmp2.p));
      double zin = 0.0, zout = 0.0;
      FSICHK(norm2(ctx, ctx->tmp1.p, &zin));
      FSICHK(norm2(ctx, ctx->tmp2.p, &zout));
      if (getenv("FSI_DEBUG_PRECOND"))
        fprintf(stderr, "[precond] self-test %d: |in| %.3e |out| %.3e  lmax solid %.4g fluid %.4g schur %.4g disp %.4g  coarse solid %.4g disp %.4g\n",
                attempt, zin, zout, ctx->lmax_s, ctx->lmax_f, ctx->lmax_p, ctx->lmax_d, ctx->sbmg_clmax, ctx->mg_clmax);
      if (std::isfinite(zout) && zout < 1e8 * zin) break;
      // a diverging Chebyshev recurrence grows exponentially with the sweep count and collapses once the interval covers
      // the spectrum; an output that is large but barely moves when the intervals widen by 1.6x is the genuine size of
      // M^-1 on this matrix (small time steps: the avf problem runs at dt = 1e-4 and answers a unit ripple with 4e9):
      // keep the estimated intervals
      if (attempt > 0 && std::isfinite(zout) && std::isfinite(prev_out) && zout > 0.25 * prev_out) {
        ctx->lmax_s = l0[0]; ctx->lmax_f = l0[1]; ctx->lmax_p = l0[2]; ctx->lmax_d = l0[3];
        break;
      }
      prev_out = zout;
      if (attempt == 7) { ctx->prec_bad = true; break; }      // reported by fsi_solve: assembling such a Jacobian is legal
      ctx->lmax_s *= 1.6; ctx->lmax_f *= 1.6; ctx->lmax_p *= 1.6; ctx->lmax_d *= 1.6;
      ctx->sbmg_clmax = std::min(ctx->sbmg_clmax * 1.6, std::max(ctx->sbmg_clmax, (double)ctx->sbmg_gersh));      // towards the row-sum bounds
      ctx->mg_clmax = std::min(ctx->mg_clmax * 1.6, std::max(ctx->mg_clmax, (double)ctx->mg_gersh));
    }
    return FSI_OK;
  }
  if (!ctx->LU.p) HIPCHK(ctx->LU.alloc(ctx->nnz));
  HIPCHK(hipMemcpyAsync(ctx->LU.p, ctx->A.p, ctx->nnz * sizeof(double), hipMemcpyDeviceToDevice, st));
  launch_ilu0_levels(st, ctx->levels, ctx->rowptr.p, ctx->cols.p, ctx->diagpos.p, ctx->LU.p, ctx->iflags.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
  ctx->have_monolithic_lu = true;
  if (flags[1] & 1) { ctx->err = "ILU(0): a row has more than 1024 entries"; return FSI_ERR_INVALID; }
  if (flags[1] & 2) { ctx->err = "ILU(0): zero or non-finite pivot"; return FSI_ERR_PIVOT; }
  return FSI_OK;
}

}  // namespace host
}  // namespace fsi
