// The field-split block preconditioner of the monolithic Jacobian: one application (precondition_block: ~210 dependent
// launches on two HIP streams) and its refresh at every new Jacobian (refresh_preconditioner: field blocks, explicit Schur
// complement, Galerkin coarse operators, eigenvalue estimates, self-test).  Kernels: fsi_block.hip.  DESIGN.md section 5.
#include "fsi_cheb.hpp"
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace {

struct CsrRef { int64_t n; const int64_t* rowptr; const int32_t* cols; const double* vals; const int64_t* diagpos; };
CsrRef ss_ref(FsiCtx* c) { return CsrRef{3 * c->nS, c->ss_rowptr.p, c->ss_cols.p, c->ss_vals.p, c->ss_diagpos.p}; }

// Chebyshev solve with a Jacobi scaling taken from (dvals, diagpos); `apply(in, out)` is the operator.  W: 3 work vectors
// (r, d, t).  Product and update are two launches, all in FP64, and every sweep is launched.
template <class Apply>
void cheb_solve_op(FsiCtx* ctx, int64_t n, Apply&& apply, const double* dvals, const int64_t* diagpos, const double* mask,
                   const double* rhs, double* x, double* W, int its, double lmax, double kappa) {
  hipStream_t st = ctx->stream;
  double *r = W, *d = W + n, *t = W + 2 * n;
  ChebSchedule gen(lmax, kappa);
  launch_cheb_init(st, n, mask, rhs, diagpos, dvals, gen.init(), x, r, d);
  run_chain(gen, its, false, [&](int, double c1, double c2) {
    apply(d, t);
    launch_cheb_step(st, n, mask, t, diagpos, dvals, c1, c2, x, r, d);
  });
}
// ... of the masked velocity block or another CSR matrix (see fsi_block.hip)
void cheb_solve(FsiCtx* ctx, const CsrRef& M, const double* mask, const double* rhs, double* x, double* W, int its,
                double lmax, double kappa) {
  cheb_solve_op(ctx, M.n, [&](const double* in, double* out) { launch_spmv(ctx->stream, M.n, M.rowptr, M.cols, M.vals, in, out); },
                M.vals, M.diagpos, mask, rhs, x, W, its, lmax, kappa);
}
// Schur operator y = (A_pp - Apv~ D^-1 A_vp) x, explicit since round 2
void schur_apply(FsiCtx* ctx, const double* in, double* out) {
  launch_spmv(ctx->stream, ctx->V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals.p, in, out, SPMV_FIELD_BLOCK);
}

// The last sweep of a Chebyshev chain is not launched: the chain's consumer adds the last direction to x (run_chain,
// fsi_cheb.hpp).  FsiTuning.experiment bit 2 launches every sweep as before.
inline bool drop_last_sweep(const FsiCtx* ctx) { return (ctx->tune.experiment & 4) == 0; }
// this application's sweep launches are timed by event pairs (the 16 applications after fsi_get_timers(reset))
inline bool sampled(const FsiCtx* ctx) { return ctx->sample_budget > 0; }

// The FP32 sweep vectors (float4 per node: r, d, t, x, rhs) in a work area of doubles, aligned for float4 loads
struct F32Work {
  float *r, *d, *t, *x, *rhs;
  F32Work(double* W, int64_t n) {
    float* F = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(W) + 15) & ~uintptr_t(15));
    r = F; d = F + n; t = F + 2 * n; x = F + 3 * n; rhs = F + 4 * n;
  }
};

// FP32 Chebyshev sweeps on a component-diagonal node-block matrix; dinv carries the Jacobi scaling and the mask.
// Returns the number of product sweeps launched.  Sampled: the first 4 sweeps of a call, 8 pairs over an application's calls.
int cheb_db_f32(FsiCtx* ctx, const float* db, const float* dinv, const double* rhs, double* x, double* W, int its,
                double lmax, double kappa, hipStream_t st) {
  const int64_t n = 4 * ctx->N2;                 // float4 per node
  const F32Work f(W, n);
  ChebSchedule gen(lmax, kappa);
  const bool fused = ctx->tiled && ctx->fused_sweeps;
  float *da = f.d, *db_ = f.t;                   // fused: d is ping-ponged, the product stays in registers; unfused: d stays in f.d
  launch_pad_init_f32(st, ctx->N2, rhs, nullptr, dinv, (float)gen.init(), f.x, f.r, f.d);      // pad + initialise in one launch
  const ChainRun run = run_chain(gen, its, drop_last_sweep(ctx), [&](int k, double c1, double c2) {
    ctx->smp_db.begin(st, sampled(ctx) && k < 4);
    if (!fused) {
      if (ctx->tiled)
        launch_spmv_tiled_f32(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, db, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr, f.d, f.t);
      else
        launch_spmv_db_f32(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, db, f.d, f.t);
      ctx->smp_db.end(st);
      launch_cheb_step_f32(st, n, f.t, dinv, (float)c1, (float)c2, f.x, f.r, f.d);
      return;
    }
    if (ctx->sweeps_fp16 && db == ctx->vv_db32.p)
      launch_sweep_tiled_h(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->vv_rec.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr,
                           dinv, (float)c1, (float)c2, da, db_, f.x, f.r);
    else if (ctx->vv_rec32.p && db == ctx->vv_db32.p)
      launch_sweep_tiled_r3(st, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->vv_rec32.p, ctx->tile_uptr.p, ctx->tile_ulist.p, nullptr,
                            dinv, (float)c1, (float)c2, da, db_, f.x, f.r);
    else
      launch_sweep_tiled_f32(st, 3, ctx->tile_nodes, ctx->N2, ctx->tile_max_nu, ctx->nadj_ptr.p, db, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                             nullptr, dinv, (float)c1, (float)c2, da, db_, f.x, f.r);
    ctx->smp_db.end(st);
    std::swap(da, db_);
  });
  launch_unpad_from_f32(st, ctx->N2, f.x, x, run.d_left ? da : nullptr);      // the unpad adds the dropped last sweep's d
  return run.launched;
}

// One application: the work vectors (ctx->blk), the two streams and what one stage hands the next
struct BlockApply {
  FsiCtx* ctx;
  int64_t n3, V, N2;
  double *rd, *rv, *rp, *vs, *tp, *dp, *dv, *td, *dd, *IW, *w3;      // IW: 10 vectors; its first 4 hold the (FP32, float4-padded) sweep work
  double *xs, *xf;                               // the solid and the fluid predictor, IW[4 n3, 6 n3)
  bool conc = false, drop;                       // two chains; every chain ends one sweep early and hands its consumer x and d
  hipStream_t sA, sB, st;                        // st: the stream of the stage being issued
  const float *dd_f32 = nullptr, *dd_d = nullptr;      // the displacement sweeps' result and direction, for the merge
  explicit BlockApply(FsiCtx* c) : ctx(c), n3(3 * c->N2), V(c->V), N2(c->N2), drop(drop_last_sweep(c)), sA(c->stream), sB(c->stream), st(c->stream) {
    double* W = c->blk.p;
    rd = W; rv = W + n3; rp = W + 2 * n3; vs = W + 3 * n3; tp = W + 4 * n3; dp = W + 5 * n3; dv = W + 6 * n3;
    td = W + 7 * n3; dd = W + 8 * n3; IW = W + 9 * n3; w3 = W + 19 * n3;
    xs = IW + 4 * n3; xf = IW + 5 * n3;
  }
  // the stages, in the order precondition_block issues them
  int solid_cycle(const F32Work& f, const float** xs_d), solid_one_level(const F32Work& f, const float** xs_d), solid_predictor();
  int fluid_predictor(const double* rhs, double* W, hipStream_t st_f), displacement_block();
  void schur_fused(bool mixed), pressure_step(), displacement_scalar();
};

// One fused sweep of the solid block on the fine level; h: the packed FP16 records may be used (the two-level cycle only)
void solid_sweep(FsiCtx* ctx, hipStream_t st, bool h, float c1, float c2, const float* din, float* dout, float* x, float* r) {
  if (h && ctx->sweeps_fp16 && ctx->sb_rec.p)
    launch_sweep_sb_h(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_rec.p, ctx->sb_binv12.p, c1, c2, din, dout, x, r);
  else if (ctx->sb_rec32.p)
    launch_sweep_sb_r(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_rec32.p, ctx->sb_binv12.p, c1, c2, din, dout, x, r);
  else
    launch_sweep_sb_b3(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, ctx->sb_binv12.p, c1, c2, din, dout, x, r);
}

// Two-level cycle (see the displacement block): smoothing on [lmax/alpha, lmax], coarse solve on the solid vertices.
// FSI_CHEB4 bit 0: the smoothing sweeps as Chebyshev polynomials of the 4th kind.  Sampled: the first 8 pre-smoothing sweeps.
int BlockApply::solid_cycle(const F32Work& f, const float** xs_d) {
  ChebSchedule gen(ctx->lmax_s, ctx->sbmg_alpha, (ctx->cheb4 & 1) != 0);
  float *dcur = f.d, *dnext = f.t;
  bool sampling = sampled(ctx);
  // gather, x = 0, first direction and the zeroed second buffer in ONE launch
  launch_solid_cycle_init(st, ctx->nS, ctx->snode.p, rv, ctx->sb_binv12.p, (float)gen.init(), f.x, f.r, f.d, f.t);
  auto sweep = [&](int, double c1, double c2) {
    ctx->smp_ss.begin(st, sampling);
    solid_sweep(ctx, st, true, (float)c1, (float)c2, dcur, dnext, f.x, f.r);
    ctx->smp_ss.end(st);
    std::swap(dcur, dnext);
  };
  const ChainRun pre = run_chain(gen, ctx->sbmg_pre, false, sweep);
  sampling = false;                              // tail sweeps are never sampled
  const int64_t nc = ctx->sbmg_nc, n4c = 4 * nc;
  float *cr = ctx->sbmg_work.p, *cd = cr + n4c, *cd2 = cr + 2 * n4c, *cx = cr + 3 * n4c, *crhs = cr + 4 * n4c;
  const bool exact = bcr_ready(ctx);
  const float* cx_d = nullptr;                   // the coarse chain's direction, when its last sweep is dropped
  launch_sbmg_restrict(st, nc, ctx->sbmg_chptr.p, ctx->sbmg_child.p, ctx->sbmg_chw.p, ctx->snode.p, ctx->rowscale.p,
                       ctx->sbmg_flag.p, ctx->sbmg_cflag.p, f.r, crhs, exact ? bcr_pos(ctx) : nullptr, exact ? bcr_rhs(ctx) : nullptr);
  if (exact) {
    // the coarse level solved exactly: block cyclic reduction over the breadth-first levels of the solid vertices, operators
    // precomputed at the Jacobian refresh (fsi_bcr.hip) - 2 log2(blocks) + 1 launches instead of sbmg_cits dependent sweeps;
    // the restriction wrote the right-hand side in the solve's own order and the prolongation reads the answer there
    FSICHK(bcr_solve(ctx, nullptr, nullptr, st));
    ctx->bcr_solves += 1;
  } else {
    ChebSchedule cgen(ctx->sbmg_clmax, ctx->sbmg_ckappa);
    launch_cheb_init_b3(st, nc, crhs, ctx->sbmg_cbinv12.p, (float)cgen.init(), cx, cr, cd);
    HIPCHK(hipMemsetAsync(cd2, 0, n4c * sizeof(float), st));
    float *ca = cd, *cb = cd2;
    const ChainRun coarse = run_chain(cgen, ctx->sbmg_cits, drop, [&](int, double c1, double c2) {
      launch_sweep_sb_b3(st, nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cbinv12.p, (float)c1, (float)c2, ca, cb, cx, cr, 1);
      std::swap(ca, cb);
    });
    if (coarse.d_left) cx_d = ca;
  }
  launch_sbmg_prolong(st, ctx->nS, ctx->sbmg_par.p, ctx->sbmg_pw.p, ctx->sbmg_flag.p, cx, dcur,     // correction as the next direction
                      exact ? bcr_pos(ctx) : nullptr, exact ? bcr_sol(ctx) : nullptr, cx_d);
  // the restart and the post-smoothing sweeps are one chain whose last sweep is left to the scatter (with sbmg_post = 0
  // that is the restart itself: x += P x_c happens there, A P x_c is not formed)
  const ChainRun tail = run_chain(gen, ctx->sbmg_post + 1, drop, sweep, true);
  if (tail.d_left) *xs_d = dcur;
  ctx->inner_its[0] += pre.launched + tail.launched;
  return FSI_OK;
}

// One-level FP32 fall-back: block-Jacobi (bj) or Jacobi scaling, product and update in one launch (fused) or two.
// Sampled: the first 8 products.
int BlockApply::solid_one_level(const F32Work& f, const float** xs_d) {
  const int64_t n = 4 * ctx->nS;                 // float4 per solid node
  const bool bj = ctx->solid_block_jacobi != 0, fused = bj && ctx->solid_fused;
  ChebSchedule gen(ctx->lmax_s, ctx->cheb_kappa_s);
  launch_gather3_f32(st, ctx->nS, ctx->snode.p, rv, f.rhs);
  if (bj) launch_cheb_init_b3(st, ctx->nS, f.rhs, ctx->sb_binv12.p, (float)gen.init(), f.x, f.r, f.d);
  else launch_cheb_init_f32(st, n, f.rhs, ctx->sb_dinv.p, (float)gen.init(), f.x, f.r, f.d);
  if (fused) HIPCHK(hipMemsetAsync(f.t, 0, n * sizeof(float), st));     // second d buffer (ping-pong), pads stay zero
  float *dcur = f.d, *dnext = f.t;
  const ChainRun run = run_chain(gen, ctx->cheb_its_s, drop, [&](int, double c1, double c2) {
    ctx->smp_ss.begin(st, sampled(ctx));
    if (fused) {
      solid_sweep(ctx, st, false, (float)c1, (float)c2, dcur, dnext, f.x, f.r);
      ctx->smp_ss.end(st);
      std::swap(dcur, dnext);
      return;
    }
    launch_spmv_sb(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, f.d, f.t);
    ctx->smp_ss.end(st);
    if (bj) launch_cheb_step_b3(st, ctx->nS, f.t, ctx->sb_binv12.p, (float)c1, (float)c2, f.x, f.r, f.d);
    else launch_cheb_step_f32(st, n, f.t, ctx->sb_dinv.p, (float)c1, (float)c2, f.x, f.r, f.d);
  });
  if (run.d_left) *xs_d = dcur;                  // (unfused sweeps keep the direction in f.d = dcur)
  ctx->inner_its[0] += run.launched;
  return FSI_OK;
}

// Solid part of the velocity predictor (elasticity-dominated, many cheap sweeps): xs on the solid nodes, zero elsewhere
int BlockApply::solid_predictor() {
  if (ctx->solid_fp32) {
    const F32Work f(IW, 4 * ctx->nS);
    const float* xs_d = nullptr;                 // the direction the scatter below adds to f.x: that of the dropped last sweep
    if (ctx->solid_block_jacobi && ctx->solid_fused && ctx->sbmg_ready) FSICHK(solid_cycle(f, &xs_d));
    else FSICHK(solid_one_level(f, &xs_d));
    // xs is written by this scatter alone (the sweeps' work areas end below it): its non-solid entries stay zero from one
    // application to the next, so the 3 N2-entry fill runs once per context instead of once per application
    if (ctx->xs_zeroed != xs) { launch_fill(st, xs, n3, 0.0); ctx->xs_zeroed = xs; }
    launch_scatter3_f32(st, ctx->nS, ctx->snode.p, f.x, xs, xs_d);
    return FSI_OK;
  }
  // all FP64 on the compact solid vectors (3 nS <= n3); sampled: the first 8 products
  double *cs_rhs = IW + 7 * n3, *cs_x = IW + 8 * n3;
  const CsrRef M = ss_ref(ctx);
  ctx->xs_zeroed = nullptr;
  ctx->inner_its[0] += ctx->cheb_its_s;
  launch_gather3(st, ctx->nS, ctx->snode.p, rv, cs_rhs);
  cheb_solve_op(ctx, M.n,
                [&](const double* in, double* out) {
                  ctx->smp_ss.begin(st, sampled(ctx));
                  launch_spmv(st, M.n, M.rowptr, M.cols, M.vals, in, out, SPMV_SOLID_BLOCK);
                  ctx->smp_ss.end(st);
                },
                M.vals, M.diagpos, nullptr, cs_rhs, cs_x, IW, ctx->cheb_its_s, ctx->lmax_s, ctx->cheb_kappa_s);
  launch_fill(st, xs, n3, 0.0);
  launch_scatter3(st, ctx->nS, ctx->snode.p, cs_x, xs);
  return FSI_OK;
}

// Fluid interior (mass-dominated) from `rhs` into xf on the stream st_f; returns the product sweeps launched.  W: the sweeps' work area.
int BlockApply::fluid_predictor(const double* rhs, double* W, hipStream_t st_f) {
  if (ctx->sweeps_fp32)
    return cheb_db_f32(ctx, ctx->vv_db32.p, ctx->vvf_dinv32.p, rhs, xf, W, ctx->cheb_its_f, ctx->lmax_f, ctx->cheb_kappa_f, st_f);
  cheb_solve_op(ctx, n3, [&](const double* in, double* out) { launch_spmv_db(st_f, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->vv_db.p, in, out); },
                ctx->Mvv.vals.p, ctx->diagpos3.p, ctx->mask_f.p, rhs, xf, W, ctx->cheb_its_f, ctx->lmax_f, ctx->cheb_kappa_f);
  return ctx->cheb_its_f;
}

// Schur sweeps, product fused with the Chebyshev update (one launch per sweep), vectors in FP64.  mixed: matrix values in
// FP16 / FP32 (k_sweep_schur_tiled / k_sweep_csr_mixed).  (All-FP32 vectors were measured in round 2: their rounding noise
// exceeds the velocity residual on a coarse mesh and the outer iteration stalls.)  Otherwise all FP64.  Sampled: the first 4.
void BlockApply::schur_fused(bool mixed) {
  double *pr = conc ? rp + V : IW, *pa = pr + V, *pb = pr + 2 * V;      // two chains: the Schur vectors live in the unused tail of rp, IW is stream A's
  // FSI_CHEB4 bit 2: the Schur sweeps as the 4th-kind polynomial (needs lmax only; see the solid block).  The all-FP64
  // sweeps ignore the bit (vaspfsi.h, cheb4)
  ChebSchedule gen(ctx->lmax_p, ctx->cheb_kappa_p, mixed && (ctx->cheb4 & 4) != 0);
  const bool tiled16 = ctx->schur_tiled && ctx->sweeps_fp16 && ctx->s_rec.p;
  launch_cheb_init(st, V, nullptr, tp, ctx->s_diagpos.p, ctx->s_vals.p, gen.init(), dp, pr, pa);
  const ChainRun run = run_chain(gen, ctx->cheb_its_p, drop, [&](int, double c1, double c2) {
    ctx->smp_sch.begin(st, sampled(ctx));
    if (mixed && tiled16)
      launch_sweep_schur_tiled(st, ctx->schur_tile, V, ctx->s_tile_max_nu, ctx->s_rowptr.p, ctx->s_rec.p, ctx->s_tile_uptr.p, ctx->s_tile_ulist.p,
                               ctx->s_dinv.p, c1, c2, pa, pb, dp, pr);
    else if (mixed)
      launch_sweep_csr_mixed(st, V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals32.p, ctx->s_diagpos.p, ctx->s_vals.p, c1, c2, pa, pb, dp, pr);
    else if (ctx->schur_tiled)      // the tiles of the FP16 form with the FP64 values: bitwise the sweep of launch_sweep_csr_f64
      launch_sweep_schur_tiled_f64(st, ctx->schur_tile, V, ctx->s_tile_max_nu, ctx->s_rowptr.p, ctx->s_vals.p, ctx->s_ploc.p,
                                   ctx->s_tile_uptr.p, ctx->s_tile_ulist.p, ctx->s_diagpos.p, c1, c2, pa, pb, dp, pr);
    else
      launch_sweep_csr_f64(st, V, ctx->s_rowptr.p, ctx->s_cols.p, ctx->s_vals.p, ctx->s_diagpos.p, c1, c2, pa, pb, dp, pr);
    ctx->smp_sch.end(st);
    std::swap(pa, pb);
  });
  // the dropped last sweep's x += d: V doubles, a launch of its own in front of the velocity correction
  if (run.d_left) launch_axpby(st, dp, 1.0, dp, 1.0, pa, V);
  ctx->inner_its[1] += run.launched;
}

// pressure: S dp = rp - Apv~ vs,  S x = App x - Apv~ D^-1 Avp x;  then the velocity correction dv
void BlockApply::pressure_step() {
  if (ctx->pv32_ok)
    launch_pres_rhs32(st, V, ctx->vrank.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->rowptr_pv.p, ctx->Apv32.p,
                      (ctx->tune.experiment & 1) ? xf : vs, rp, tp);      // experiment bit 0: pressure rhs from the FLUID predictor only
  else
    launch_pres_rows(st, V, ctx->rowptr_pp.p, ctx->cols_pp.p, ctx->App.p, nullptr, 0.0, ctx->rowptr_pv.p, ctx->cols_pv.p,
                     ctx->Apv.p, vs, -1.0, rp, 1.0, tp);
  const bool mixed = ctx->schur_fp32 && ctx->s_vals32.p;
  if (ctx->cheb_its_p > 0 && (mixed || ctx->fused_sweeps)) {
    schur_fused(mixed);
  } else if (ctx->cheb_its_p > 0) {              // product and update as two launches, every sweep launched; sampled: the first 4 products
    cheb_solve_op(ctx, V,
                  [&](const double* in, double* out) {
                    ctx->smp_sch.begin(st, sampled(ctx));
                    schur_apply(ctx, in, out);
                    ctx->smp_sch.end(st);
                  },
                  ctx->s_vals.p, ctx->s_diagpos.p, nullptr, tp, dp, IW, ctx->cheb_its_p, ctx->lmax_p, ctx->cheb_kappa_p);
    ctx->inner_its[1] += ctx->cheb_its_p;
  }
  if (ctx->pv32_ok)
    launch_vel_correct32(st, N2, ctx->padj_ptr.p, ctx->padj.p, ctx->Avp32.p, dp, ctx->vv_dinv.p, vs, dv);
  else
    launch_vel_correct(st, n3, ctx->rowptr_vp.p, ctx->cols_vp.p, ctx->Avp.p, dp, ctx->diagpos3.p, ctx->Mvv.vals.p, vs, dv, ctx->vv_dinv.p);
}

// Jacobi-scaled system  (D^-1 A_dd) dd = D^-1 td  with the one-number-per-node-pair operator, in FP32: a two-level cycle
// (Chebyshev smoothing on [lmax/alpha, lmax], coarse solve on the vertex graph, smoothing again; FSI_CHEB4 bit 1: 4th-kind
// smoothing sweeps, see the solid block) or, without a coarse level, one chain.  Sampled: the first 4 products of the
// pre-smoothing or of the one chain.
void BlockApply::displacement_scalar() {
  const int64_t n = 4 * N2;
  const F32Work f(IW, n);
  const bool fused = ctx->tiled && ctx->fused_sweeps;
  float *dcur = f.d, *dnext = f.t;               // fused sweeps ping-pong the direction; f.t is otherwise the product (dcur stays f.d)
  bool sampling = sampled(ctx);
  // one sweep: product + Chebyshev update (one launch when fused)
  auto sweep = [&](int, double c1, double c2) {
    ctx->smp_sc.begin(st, sampling);
    if (!fused) {
      if (ctx->tiled)
        launch_spmv_tiled_f32(st, 1, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_chat.p, ctx->tile_ploc.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                              ctx->dd_rowflag.p, f.d, f.t);
      else
        launch_spmv_sc_f32(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_chat.p, ctx->dd_rowflag.p, f.d, f.t);
      ctx->smp_sc.end(st);
      launch_cheb_step_f32(st, n, f.t, ctx->ones32.p, (float)c1, (float)c2, f.x, f.r, f.d);
      return;
    }
    if (ctx->sweeps_fp16)
      launch_sweep_tiled_h(st, 1, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_rec.p, ctx->tile_uptr.p, ctx->tile_ulist.p,
                           ctx->dd_rowflag.p, nullptr, (float)c1, (float)c2, dcur, dnext, f.x, f.r);
    else      // k_sweep_tiled_f32<1> with two rows ahead in flight (same arrays, same sums)
      launch_sweep_tiled_a1(st, ctx->tile_nodes, N2, ctx->tile_max_nu, ctx->nadj_ptr.p, ctx->dd_chat.p, ctx->tile_ploc.p, ctx->tile_uptr.p,
                            ctx->tile_ulist.p, ctx->dd_rowflag.p, nullptr, (float)c1, (float)c2, dcur, dnext, f.x, f.r);
    ctx->smp_sc.end(st);
    std::swap(dcur, dnext);
  };
  ChainRun last{0, false};
  if (ctx->mg_ready) {
    ChebSchedule gen(ctx->lmax_d, ctx->mg_alpha, (ctx->cheb4 & 2) != 0);
    launch_pad_init_f32(st, N2, td, ctx->dd_dinv32.p, ctx->ones32.p, (float)gen.init(), f.x, f.r, f.d);      // Jacobi scaling + initialise
    const ChainRun pre = run_chain(gen, ctx->mg_pre, false, sweep);
    sampling = false;                            // tail sweeps are never sampled
    const int64_t nc = ctx->mg_nc, n4c = 4 * nc;
    float *cr = ctx->mg_work.p, *cd = cr + n4c, *ct = cr + 2 * n4c, *cx = cr + 3 * n4c, *crhs = cr + 4 * n4c;
    ChebSchedule cgen(ctx->mg_clmax, ctx->mg_ckappa);
    // restriction and the coarse recurrence's start (x = 0, r = rhs, d = rhs / theta) in one launch
    launch_mg_restrict(st, nc, ctx->mg_chptr.p, ctx->mg_child.p, ctx->mg_chw.p, ctx->mg_d0.p, f.r, ctx->mg_dcinv4.p, crhs,
                       (float)cgen.init(), cx, cr, cd);
    float *ca = cd, *cb = ct;
    const ChainRun coarse = run_chain(cgen, ctx->mg_cits, drop, [&](int, double c1, double c2) {
      if (ctx->fused_sweeps) {
        launch_sweep_sc_f32(st, nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, (float)c1, (float)c2, ca, cb, cx, cr);
        std::swap(ca, cb);
      } else {
        launch_spmv_sc_f32(st, nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, cd, ct);
        launch_cheb_step_f32(st, n4c, ct, ctx->mg_cones.p, (float)c1, (float)c2, cx, cr, cd);
      }
    });
    // the coarse chain's direction for the prolongation, when its last sweep is dropped (unfused coarse sweeps keep it in cd = ca)
    launch_mg_prolong(st, N2, ctx->mg_par.p, ctx->mg_pw.p, ctx->mg_d0.p, cx, dcur, coarse.d_left ? ca : nullptr);   // correction as the next direction
    // restart + post-smoothing: one chain, its last sweep left to the merge (with mg_post = 0 the restart itself, see the solid cycle)
    last = run_chain(gen, ctx->mg_post + 1, drop, sweep, true);      // x += P x_c, r -= C P x_c, restart
    ctx->inner_its[2] += pre.launched + last.launched;
  } else {
    ChebSchedule gen(ctx->lmax_d, ctx->cheb_kappa_d);
    launch_pad_init_f32(st, N2, td, ctx->dd_dinv32.p, ctx->ones32.p, (float)gen.init(), f.x, f.r, f.d);
    last = run_chain(gen, ctx->cheb_its_d, drop, sweep);
    ctx->inner_its[2] += last.launched;
  }
  if (last.d_left) dd_d = dcur;                // the displacement chain's direction, added by the merge (dropped last sweep)
  dd_f32 = f.x;                                // the merge takes the displacement part straight from the sweeps' result
  if (ctx->debug_prec_apply > 0) launch_unpad_from_f32(st, N2, f.x, dd, dd_d);
}

int BlockApply::displacement_block() {
  if (ctx->adv_is_db) {
    // dd_early: the displacement block sees the solid PREDICTOR instead of the corrected velocity - what it has when its chain
    // runs beside the pressure step instead of after it
    // r_d - A_dv dv in place in r_d (nothing else reads it after the split): A_dv has entries in the rows of solid nodes only
    // (adv_solid_only: verified at every refresh)
    const double* vsrc = (ctx->dd_early || conc) ? xs : dv;
    if (!(ctx->tune.experiment & 2)) {           // (experiment bit 1: displacement block without any velocity coupling)
      if (ctx->adv_solid_only)
        launch_db_rows_sub(st, ctx->nS, ctx->snode.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->adv_db.p, ctx->adv_rowmask.p, vsrc, rd);
      else {
        launch_spmv_db(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->adv_db.p, vsrc, w3, ctx->adv_rowmask.p);
        launch_axpby(st, rd, 1.0, rd, -1.0, w3, n3);
      }
    }
    td = rd;
  } else {
    launch_residual_csr(st, n3, ctx->rowptr3.p, ctx->cols3.p, ctx->Adv.p, dv, rd, td);
  }
  if (ctx->cheb_its_d <= 0) return FSI_OK;
  if (ctx->dd_is_scalar && ctx->sweeps_fp32) {
    displacement_scalar();
  } else if (ctx->dd_is_db && ctx->sweeps_fp32) {
    ctx->inner_its[2] += cheb_db_f32(ctx, ctx->dd_db32.p, ctx->dd_dinv32.p, td, dd, IW, ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d, st);
  } else if (ctx->dd_is_db) {
    ctx->inner_its[2] += ctx->cheb_its_d;
    cheb_solve_op(ctx, n3, [&](const double* in, double* out) { launch_spmv_db(st, N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p, in, out); },
                  ctx->Mdd.vals.p, ctx->diagpos3.p, nullptr, td, dd, IW, ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d);
  } else {
    ctx->inner_its[2] += ctx->cheb_its_d;
    cheb_solve(ctx, CsrRef{n3, ctx->rowptr3.p, ctx->cols3.p, ctx->Mdd.vals.p, ctx->diagpos3.p}, nullptr, td, dd, IW,
               ctx->cheb_its_d, ctx->lmax_d, ctx->cheb_kappa_d);
  }
  return FSI_OK;
}

// FSI_DEBUG_PRECOND=2: non-finite entries of the parts, first applications only
void debug_print_parts(const BlockApply& a) {
  auto bad = [&](const double* p, int64_t n) { std::vector<double> h(n); (void)hipMemcpy(h.data(), p, n * sizeof(double), hipMemcpyDeviceToHost);
                                                int64_t b = 0; double m = 0.0; for (double v : h) { if (!std::isfinite(v)) b++; else m = std::max(m, std::fabs(v)); }
                                                return std::make_pair(b, m); };
  const auto bt = bad(a.tp, a.V), bp = bad(a.dp, a.V), bv = bad(a.dv, a.n3), bd = bad(a.dd, a.n3), bs = bad(a.vs, a.n3);
  fprintf(stderr, "[precond] apply: rhs_p max %.3e (%lld bad)  dp max %.3e (%lld bad)  v* max %.3e (%lld bad)  dv max %.3e (%lld bad)  dd max %.3e (%lld bad)\n",
          bt.second, (long long)bt.first, bp.second, (long long)bp.first, bs.second, (long long)bs.first, bv.second, (long long)bv.first, bd.second, (long long)bd.first);
}

}  // namespace

namespace fsi {
namespace host {

// The two-chain condition of precondition_block (see there); the test shim reads it too.
bool block_two_chains(const FsiCtx* ctx) {
  return ctx->prec_streams && ctx->stream2 && ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused && ctx->sbmg_ready &&
         ctx->sweeps_fp32 && ctx->tiled && ctx->fused_sweeps && ctx->cheb_its_p > 0 &&
         ((ctx->schur_fp32 == 1 && ctx->s_vals32.p) || ctx->schur_fp32 == 0) &&      // (round 5: also with the all-FP64 Schur sweeps - the FP64-storage mode ran its ~5 ms application as ONE chain)
         ctx->pv32_ok && ctx->adv_is_db && ctx->cheb_its_d > 0 && ctx->dd_is_scalar && 4 * ctx->V <= 3 * ctx->N2 && ctx->debug_prec_apply == 0;
}

// z = M^-1 r with the approximate block factorisation (see fsi_block.hip):  (v,p) by SIMPLE with the d-eliminated
// velocity block, then d.
int precondition_block(FsiCtx* ctx, const double* r, double* z) {
  BlockApply a(ctx);
  const int64_t n3 = a.n3, V = a.V, N2 = a.N2;
  // Two chains side by side (prec_streams; default configuration only: FP32 solid cycle, FP32 fluid sweeps, FP16 / FP32 Schur
  // sweeps with FP64 vectors, scalar displacement block).  The application is a chain of ~210 dependent launches, most of them
  // short of filling the chip (latency- and issue-bound sweeps on 0.1 - 0.6 GB of data), and its dependences are fewer than
  // its order: the fluid predictor does not need the solid one (block Jacobi instead of Gauss-Seidel between the two parts:
  // same Krylov counts, measured), and the displacement block needs the velocity on the SOLID rows only, where the pressure
  // correction is small (dd_early: measured).  Stream A (the solver stream): split, solid predictor, displacement block,
  // merge.  Stream B: fluid predictor, then - once the solid predictor is there - pressure right-hand side, Schur sweeps,
  // velocity correction.  Work vectors of the two chains are disjoint: the solid and displacement sweeps use IW[0, 4 n3),
  // the fluid sweeps IW[6 n3, 10 n3), the Schur sweeps the unused tail of rp (V of its n3 entries carry r_p).
  a.conc = block_two_chains(ctx);
  // (the applications whose sweep launches are timed by event pairs issue both chains on the solver stream - the same arithmetic in
  // the same order per chain, and a pair brackets its kernel alone)
  if (a.conc && !sampled(ctx)) a.sB = ctx->stream2;
  const bool conc = a.conc;
  hipStream_t sA = a.sA, sB = a.sB;
  int sweeps_f = 0;                              // product sweeps launched by the fluid predictor
  launch_split(sA, N2, V, r, a.rd, a.rv, a.rp);
  if (conc) { HIPCHK(hipEventRecord(ctx->ev_split, sA)); HIPCHK(hipStreamWaitEvent(sB, ctx->ev_split, 0)); }
  // velocity predictor: block Gauss-Seidel solid -> fluid interior; two chains: block Jacobi, and stream B is issued first -
  // the fluid predictor straight from r_v (no coupling to the solid predictor), work area IW[6 n3, 10 n3)
  if (conc) sweeps_f = a.fluid_predictor(a.rv, a.IW + 6 * n3, sB);
  FSICHK(a.solid_predictor());
  if (conc) {
    // when the solid predictor is there, the rest of the pressure step follows on B while A goes on to the displacement block
    HIPCHK(hipEventRecord(ctx->ev_solid, sA));
    HIPCHK(hipStreamWaitEvent(sB, ctx->ev_solid, 0));
    a.st = sB;
  } else {
    // rhs of the fluid part: rv - Avv~ xs; xs lives on the solid nodes, the fluid solve masks the solid rows, so only
    // the fluid rows with solid columns differ from rv
    double* rhs2 = a.IW + 6 * n3;
    launch_copy(sA, rhs2, a.rv, n3);
    if (!ctx->vel_jacobi)      // (vel_jacobi: block Jacobi instead of Gauss-Seidel between the solid and the fluid part of the predictor)
      launch_residual_rows(sA, ctx->nfs, ctx->fs_rows.p, ctx->fs_ptr.p, ctx->fs_col.p, ctx->fs_src.p, ctx->Mvv.vals.p, a.xs, a.rv, rhs2);
    sweeps_f = a.fluid_predictor(rhs2, a.IW, sA);
  }
  launch_axpby(a.st, a.vs, 1.0, a.xs, 1.0, a.xf, n3);
  ctx->inner_its[0] += sweeps_f;                 // (the solid part counted its own sweeps)
  a.pressure_step();
  if (conc) { HIPCHK(hipEventRecord(ctx->ev_b, sB)); a.st = sA; }      // the rest (displacement block) is stream A's, behind the solid predictor
  FSICHK(a.displacement_block());
  if (conc) HIPCHK(hipStreamWaitEvent(sA, ctx->ev_b, 0));
  if (a.dd_f32) launch_merge_f32d(a.st, N2, V, a.dd_f32, a.dv, a.dp, z, a.dd_d);
  else launch_merge(a.st, N2, V, a.dd, a.dv, a.dp, z);
  if (ctx->debug_prec_apply > 0) { ctx->debug_prec_apply -= 1; debug_print_parts(a); }
  ctx->inner_calls += 1;
  if (ctx->sample_budget > 0) ctx->sample_budget -= 1;
  for (SweepSamples* s : {&ctx->smp_sc, &ctx->smp_sch, &ctx->smp_db, &ctx->smp_ss}) s->flush();      // the sampled launch durations of this application
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
// largest eigenvalue of S A by power iteration from a pseudo-random start (rich in element-scale modes): `apply(in, out)` is
// the operator, `scale(y)` the scaling S in place (Jacobi: mask D^-1 . mask, or the solid block's 3x3 inverses).  W: 2 vectors.
template <class Apply, class Scale>
int power_lmax_op(FsiCtx* ctx, int64_t n, Apply&& apply, Scale&& scale, const double* mask, double* W, double* out) {
  hipStream_t st = ctx->stream;
  double *x = W, *y = W + n;
  launch_mask_ripple(st, n, mask, x);
  double lam = 1.0;
  for (int k = 0; k < 40; ++k) {
    apply(x, y);
    scale(y);
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
// the Jacobi scaling mask D^-1 . mask taken from (dvals, diagpos)
auto jacobi_scale(FsiCtx* ctx, int64_t n, const double* mask, const int64_t* diagpos, const double* dvals) {
  return [=](double* y) { launch_mask_scale(ctx->stream, n, mask, diagpos, dvals, y); };
}
int power_lmax(FsiCtx* ctx, const CsrRef& M, const double* mask, double* W, double* out) {
  return power_lmax_op(ctx, M.n, [&](const double* in, double* o) { launch_spmv(ctx->stream, M.n, M.rowptr, M.cols, M.vals, in, o); },
                       jacobi_scale(ctx, M.n, mask, M.diagpos, M.vals), mask, W, out);
}

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

// A coarse level after its Galerkin product and coarse_finish: is it usable (no flag of `bad` raised, a finite positive
// largest row sum), and its Chebyshev bound - the Gershgorin row sum or, with coarse_power, the power iteration's estimate.
// exact(&power) runs on a usable level before the estimate and may clear `power` (the solid level solved exactly needs none).
template <class Sweep, class Exact>
int coarse_level_ready(FsiCtx* ctx, const char* name, int32_t bad, int64_t nc, float* work, Sweep&& sweep, Exact&& exact,
                       bool* ready, double* clmax, float* gersh) {
  int32_t flags[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(flags, ctx->iflags.p, sizeof flags, hipMemcpyDeviceToHost));
  float rowmax;
  std::memcpy(&rowmax, &flags[2], sizeof rowmax);
  *ready = !(flags[1] & bad) && std::isfinite(rowmax) && rowmax > 0.f;
  *clmax = *gersh = rowmax;   // Gershgorin bound of the scaled coarse operator
  bool power = *ready && ctx->coarse_power;
  if (*ready) FSICHK(exact(&power));
  if (power) {
    double lam = rowmax;
    FSICHK(coarse_power_lmax(ctx, nc, work, sweep, rowmax, &lam));
    if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] %s coarse level: lmax %.3f by power iteration (Gershgorin bound %.3f)\n", name, lam, (double)rowmax);
    *clmax = lam;
  }
  HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), ctx->stream));
  return FSI_OK;
}

// The field blocks of the Jacobian, the explicit Schur complement and what the application's branches are chosen by:
// A_dd / A_dv per component, A_dv in solid rows only, the scalar form of the displacement block
int extract_field_blocks(FsiCtx* ctx) {
  hipStream_t st = ctx->stream;
  int32_t flags[4] = {0, 0, 0, 0};
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
  return FSI_OK;
}

// The displacement block (solid mass + mesh Laplacian with a constant coefficient) does not change from one Jacobian
// to the next for the forms VaSP uses: what is derived from it alone - its coarse operator here, its eigenvalue
// estimate below - is kept while a checksum of the block's values (sum of squares, one pass) stays the same.
// Three numbers: the sum of squares, a sum with index-hashed weights (sign changes, permuted entries, entries
// far below the largest one) and the same hashed sum over the row scaling of the d rows, which the Galerkin product
// takes as a separate input.  fsi_get_timers counts the hits (dd_cache_hits).
int displacement_level(FsiCtx* ctx) {
  hipStream_t st = ctx->stream;
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
  if (mg_keep || !(ctx->dd_mg && ctx->dd_is_scalar && ctx->sweeps_fp32 && ctx->mg_nc > 0)) return FSI_OK;
  // Galerkin coarse operator of the displacement block, A_c = P^T A0 P, and its Jacobi-scaled single-precision form
  HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(ctx->mg_Ac.p, 0, ctx->mg_cnnz * sizeof(double), st));
  launch_mg_d0(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p, ctx->rowscale.p, ctx->dd_rowflag.p, ctx->mg_d0.p, ctx->iflags.p);
  launch_mg_rap(st, ctx->mg_nc, ctx->mg_chptr.p, ctx->mg_child.p, ctx->mg_chw.p, ctx->nadj_ptr.p, ctx->nadj.p, ctx->dd_db.p,
                ctx->rowscale.p, ctx->dd_rowflag.p, ctx->mg_par.p, ctx->mg_pw.p, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_Ac.p,
                ctx->iflags.p);
  launch_mg_coarse_finish(st, ctx->mg_nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_Ac.p, ctx->mg_cfine.p, ctx->dd_rowflag.p,
                          ctx->mg_cc.p, ctx->mg_cflag.p, ctx->mg_dcinv4.p, ctx->iflags.p + 2);
  return coarse_level_ready(ctx, "displacement", 32 | 64, ctx->mg_nc, ctx->mg_work.p,
                            [&](const float* din, float* dout, float* x, float* r) {
                              launch_sweep_sc_f32(st, ctx->mg_nc, ctx->mg_cptr.p, ctx->mg_ccol.p, ctx->mg_cc.p, ctx->mg_cflag.p, 0.f, 1.f, din, dout, x, r);
                            },
                            [](bool*) { return (int)FSI_OK; }, &ctx->mg_ready, &ctx->mg_clmax, &ctx->mg_gersh);
}

// What the sweeps read: FP32 copies, packed records and scalings of the displacement, fluid and solid blocks
int pack_sweep_records(FsiCtx* ctx) {
  hipStream_t st = ctx->stream;
  const int64_t npairs = (int64_t)ctx->dd_db.n / 3;
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
  return FSI_OK;
}

// Galerkin coarse operator of the solid block on the solid vertices, and its exact solve where that is switched on
int solid_level(FsiCtx* ctx) {
  hipStream_t st = ctx->stream;
  ctx->sbmg_ready = false;
  if (!(ctx->solid_mg && ctx->sbmg_nc > 0 && ctx->solid_fp32 && ctx->solid_block_jacobi && ctx->solid_fused)) return FSI_OK;
  HIPCHK(hipMemsetAsync(ctx->iflags.p, 0, 4 * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(ctx->sbmg_cvals.p, 0, 9 * ctx->sbmg_nblk * sizeof(float), st));
  launch_sbmg_flags(st, ctx->nS, ctx->sb_ptr.p, ctx->sb_col.p, ctx->sb_vals.p, ctx->sbmg_flag.p);
  launch_sbmg_rap(st, ctx->sbmg_nc, ctx->sbmg_chptr.p, ctx->sbmg_child.p, ctx->sbmg_chw.p, ctx->sb_ptr.p, ctx->sb_col.p,
                  ctx->sb_vals.p, ctx->snode.p, ctx->rowscale.p, ctx->sbmg_flag.p, ctx->sbmg_par.p, ctx->sbmg_pw.p,
                  ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->iflags.p);
  launch_sbmg_coarse_finish(st, ctx->sbmg_nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cfine.p,
                            ctx->sbmg_flag.p, ctx->sbmg_cbinv12.p, ctx->sbmg_cflag.p, ctx->iflags.p + 2);
  FSICHK(coarse_level_ready(ctx, "solid", 64, ctx->sbmg_nc, ctx->sbmg_work.p,
                            [&](const float* din, float* dout, float* x, float* r) {
                              launch_sweep_sb_b3(st, ctx->sbmg_nc, ctx->sbmg_cptr.p, ctx->sbmg_ccol.p, ctx->sbmg_cvals.p, ctx->sbmg_cbinv12.p, 0.f, 1.f, din, dout, x, r, 1);
                            },
                            [&](bool* power) {
                              if (ctx->bcr && ctx->solid_coarse_exact) FSICHK(bcr_refresh(ctx));      // exact coarse solve: operators of the new matrix
                              if (bcr_ready(ctx)) *power = false;
                              return (int)FSI_OK;
                            },
                            &ctx->sbmg_ready, &ctx->sbmg_clmax, &ctx->sbmg_gersh));
  if (getenv("FSI_DEBUG")) fprintf(stderr, "[fsi] solid two-level: %lld coarse nodes, clmax %.3f, ready %d\n", (long long)ctx->sbmg_nc, ctx->sbmg_gersh, (int)ctx->sbmg_ready);
  return FSI_OK;
}

// Largest eigenvalues of the four scaled blocks (the tops of the Chebyshev intervals), then the Schur complement's sweep forms
int eigenvalue_estimates(FsiCtx* ctx) {
  hipStream_t st = ctx->stream;
  if (ctx->solid_block_jacobi && ctx->solid_fp32) {      // largest eigenvalue of D_b^-1 A_SS
    const CsrRef M = ss_ref(ctx);
    FSICHK(power_lmax_op(ctx, M.n, [&](const double* in, double* o) { launch_spmv(st, M.n, M.rowptr, M.cols, M.vals, in, o, SPMV_SOLID_BLOCK); },
                         [&](double* y) { launch_block_scale_d(st, ctx->nS, ctx->sb_binv9.p, y); }, nullptr, ctx->blk.p, &ctx->lmax_s));
  } else {
    FSICHK(power_lmax(ctx, ss_ref(ctx), nullptr, ctx->blk.p, &ctx->lmax_s));
  }
  FSICHK(power_lmax_op(ctx, 3 * ctx->N2, [&](const double* in, double* o) { launch_spmv_db(st, ctx->N2, ctx->nadj_ptr.p, ctx->nadj.p, ctx->vv_db.p, in, o); },
                       jacobi_scale(ctx, 3 * ctx->N2, ctx->mask_f.p, ctx->diagpos3.p, ctx->Mvv.vals.p), ctx->mask_f.p, ctx->blk.p, &ctx->lmax_f));
  // its 40 power iterations on a 3 N2-row CSR matrix were 60 ms of every refresh: kept while the block is unchanged (dd_same)
  if (ctx->lmax_d_cached > 0.0 && ctx->dd_same) {
    ctx->lmax_d = ctx->lmax_d_cached;
  } else {
    FSICHK(power_lmax(ctx, CsrRef{3 * ctx->N2, ctx->rowptr3.p, ctx->cols3.p, ctx->Mdd.vals.p, ctx->diagpos3.p}, nullptr,
                      ctx->blk.p, &ctx->lmax_d));
    ctx->lmax_d_cached = ctx->lmax_d;
  }
  FSICHK(power_lmax_op(ctx, ctx->V, [&](const double* in, double* o) { schur_apply(ctx, in, o); },
                       jacobi_scale(ctx, ctx->V, nullptr, ctx->s_diagpos.p, ctx->s_vals.p), nullptr, ctx->blk.p, &ctx->lmax_p));
  if (ctx->schur_fp32) {
    if (!ctx->s_vals32.p) HIPCHK(ctx->s_vals32.alloc(ctx->s_vals.n));
    launch_to_f32(st, (int64_t)ctx->s_vals.n, ctx->s_vals.p, ctx->s_vals32.p);
    if (ctx->schur_tiled && ctx->sweeps_fp16) {
      if (!ctx->s_rec.p) { HIPCHK(ctx->s_rec.alloc(ctx->s_vals.n)); HIPCHK(ctx->s_dinv.alloc(ctx->V)); }
      launch_pack_h1(st, (int64_t)ctx->s_vals.n, ctx->s_vals32.p, ctx->s_ploc.p, ctx->s_rec.p);
      launch_diag_inverse(st, ctx->V, ctx->s_diagpos.p, ctx->s_vals.p, ctx->s_dinv.p);
    }
  }
  return FSI_OK;
}

// self-test: a Chebyshev interval that misses the top of a spectrum (non-normal blocks at rough states) blows up;
// widen the intervals until one application to a rippled vector stays finite and bounded
int self_test(FsiCtx* ctx) {
  ctx->prec_bad = false;
  double prev_out = 0.0;
  const double l0[4] = {ctx->lmax_s, ctx->lmax_f, ctx->lmax_p, ctx->lmax_d};
  for (int attempt = 0; attempt < 8; ++attempt) {
    launch_mask_ripple(ctx->stream, ctx->ndof, nullptr, ctx->tmp1.p);
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
}  // namespace

namespace fsi {
namespace host {

int refresh_preconditioner(FsiCtx* ctx) {
  Phase ph(ctx, &ctx->t_fac);
  ctx->xs_zeroed = nullptr;          // (the refresh uses ctx->blk as scratch: the next application zeroes its solid-predictor vector again)
  hipStream_t st = ctx->stream;
  if (!ctx->coloured && ctx->precond != 0) {
    ctx->err = "the monolithic ILU(0) preconditioner needs the multicolour node ordering: create the context with FSI_ORDER=colour";
    return FSI_ERR_INVALID;
  }
  if (ctx->precond == 0) {
    FSICHK(extract_field_blocks(ctx));
    FSICHK(displacement_level(ctx));
    FSICHK(pack_sweep_records(ctx));
    FSICHK(solid_level(ctx));
    FSICHK(eigenvalue_estimates(ctx));
    return self_test(ctx);
  }
  int32_t flags[4] = {0, 0, 0, 0};
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
