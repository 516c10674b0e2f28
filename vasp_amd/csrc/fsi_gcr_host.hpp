// The host side of the recycled GCR (solve_gcr, fsi_krylov.hip) that needs no device: the slot bookkeeping of the store, the
// layout of the pinned staging buffer, the coefficient algebra of the directions that are not explicit yet, and the policies
// of a cycle and of a solve.  Plain C++: the solver and the test shim read the same arithmetic.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace fsi {

constexpr int GCR_WINDOW = 32;        // FP32 basis: columns of the FP64 window of the current cycle's directions (KQh)
constexpr int GCR_FLUSH_BATCH = 32;   // directions made before they become explicit: rows of gcr_cn / gcr_slots (launch_gcr_flush takes <= 32)
// a full store keeps its first cap - ring directions and rotates the rest, retiring `batch` of them at a time
inline int64_t gcr_ring(int64_t cap) { return std::min<int64_t>(64, cap / 2); }
inline int gcr_retire_batch(int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>(32, cap / 4)); }
// device coefficients of a pass over `cols` columns: the coefficients, |w|^2, w.r, and one number that rides along
inline size_t gcr_coef_len(int64_t cols) { return (size_t)cols + 4; }

// Slots of the store: which columns of KQ / KZ hold a direction, and which of them the FP64 window mirrors.
struct GcrStore {
  int64_t cap = 0;
  int64_t hw = 0;                      // slots in use (columns scanned by the kernels), <= cap
  int64_t made = 0;                    // directions made since the last Jacobian (statistics / ring age)
  std::vector<int64_t> born;           // [cap] creation index of the direction in each slot (-1: free)
  std::vector<int32_t> free;           // free slots (retired in batches when the store is full)
  std::vector<int32_t> hot_slots;      // [GCR_WINDOW] slot of each window column (-1: empty)
  int hot_next = 0;
  int32_t fresh = -1;                  // the slot hw - 1 while it has been taken beyond the high-water mark and its q column not written yet

  void init(int64_t cap_) {
    cap = cap_;
    born.assign((size_t)cap, -1);
    hot_slots.assign(GCR_WINDOW, -1);
    reset();
  }
  void reset() {
    clear_window();
    made = 0;
    hw = 0;
    fresh = -1;
    free.clear();
    std::fill(born.begin(), born.end(), (int64_t)-1);
  }
  bool full() const { return free.empty() && hw == cap; }
  int64_t kept() const { return hw - (int64_t)free.size(); }
  // a slot for a new direction: the free list's back, else the high-water mark.  *clear: the slot's q column has never been
  // written (a retired column was zeroed when it left).  It is the last of the hw columns, and the Gram-Schmidt kernels are
  // told to take it as zeros without reading it - lead() - until the update kernel has written it (set_born); an iteration
  // that leaves before that hands the slot to abandon() and zeroes the column it names, so that no later scan meets garbage.
  int take(bool* clear) {
    *clear = free.empty();
    if (!free.empty()) {
      const int slot = free.back();
      free.pop_back();
      return slot;
    }
    hw += 1;
    fresh = (int32_t)hw - 1;
    return (int)hw - 1;
  }
  // the leading columns that hold data (directions, or the zeros of retired ones): all hw but an unwritten fresh slot
  int64_t lead() const { return fresh >= 0 ? hw - 1 : hw; }
  void set_born(int slot) {
    born[slot] = made;
    made += 1;
    if (slot == fresh) fresh = -1;
  }
  // the iteration that took `slot` ends without writing it: the column to zero now, or -1 (a retired slot's column is zero already).
  // The slot stays taken, as it always did: hw, and with it every count of columns scanned, moves as before.
  int abandon(int slot) {
    if (slot < 0 || slot != fresh) return -1;
    fresh = -1;
    return slot;
  }
  // retire the oldest directions of the rotating part (everything explicit: call after a flush); the caller zeroes the columns
  std::vector<int32_t> retire(int batch) {
    const int64_t protect = cap - gcr_ring(cap);          // the first `protect` directions of this Jacobian stay: they resolved the hardest modes
    std::vector<std::pair<int64_t, int32_t>> cand;
    for (int64_t sidx = 0; sidx < hw; ++sidx)
      if (born[sidx] >= protect) cand.emplace_back(born[sidx], (int32_t)sidx);
    std::sort(cand.begin(), cand.end());
    std::vector<int32_t> out;
    for (int k = 0; k < batch && k < (int)cand.size(); ++k) {
      const int32_t sidx = cand[k].second;
      born[sidx] = -1;
      free.push_back(sidx);
      out.push_back(sidx);
    }
    return out;
  }
  // FP64 window: directions of the current cycle only
  void clear_window() {
    std::fill(hot_slots.begin(), hot_slots.end(), -1);
    hot_next = 0;
  }
  // columns [0, n) of the window are in use (it fills from 0 and then turns into a ring)
  int window_cols() const {
    int nh = 0;
    for (int k = 0; k < GCR_WINDOW; ++k)
      if (hot_slots[k] >= 0) nh = k + 1;
    return nh;
  }
  int window_put(int slot) {           // returns the column the exact q goes into
    const int col = hot_next;
    hot_slots[col] = slot;
    hot_next = (hot_next + 1) % GCR_WINDOW;
    return col;
  }
  std::vector<int> window_drop_retired() {      // a retired direction leaves the window too; returns the columns to zero
    std::vector<int> out;
    for (int k = 0; k < GCR_WINDOW; ++k)
      if (hot_slots[k] >= 0 && born[hot_slots[k]] < 0) {
        hot_slots[k] = -1;
        out.push_back(k);
      }
    return out;
  }
};

// The pinned staging buffer the host reads a pass's results from.  A pass over m columns of the store leaves the m
// coefficients at 0, |w|^2 and w.r behind them, and behind those what rides along: the lagged |r|^2 of a partitioned pass, or
// in a single context the update kernel's |w'|^2 and w'.r.  The window's pass has an area of its own behind all that.
struct GcrStaging {
  int64_t cap;
  static int64_t sums(int m) { return m; }
  static int64_t lagged(int m) { return m + 2; }
  static int64_t updated(int m) { return m + 2; }
  int64_t window() const { return (int64_t)gcr_coef_len(cap); }
  size_t size() const { return gcr_coef_len(cap) + gcr_coef_len(GCR_WINDOW); }
};

// One solve cycle's bookkeeping: the directions made since the last flush are p_k = sum_j cn[k][j] Z_j (Z_j explicit
// for older slots, the raw preconditioned vector for the new ones) and x = x_flushed + sum_j y[j] Z_j.
struct GcrCycle {
  std::vector<double> y;                 // [cap]
  std::vector<std::vector<double>> cn;   // knew columns of length cap
  std::vector<int32_t> slots;            // their slots
  explicit GcrCycle(int64_t cap) : y((size_t)cap, 0.0) {}
  int knew() const { return (int)slots.size(); }
  // the direction stored in `slot` after orthogonalisation against m columns with coefficients htot:
  // p = (z - sum_j h_j p_j) / wn on the store, and x += alpha p
  void add(int slot, const double* htot, int m, double wn, double alpha) {
    const int64_t cap = (int64_t)y.size();
    std::vector<double> c((size_t)cap, 0.0);
    c[slot] = 1.0;
    for (int j = 0; j < m; ++j) {
      const double hj = htot[j];
      if (hj == 0.0 || j == slot) continue;
      bool is_new = false;
      for (size_t k = 0; k < slots.size(); ++k)
        if (slots[k] == j) {                 // a direction of this cycle: expand it on the store
          for (int64_t i = 0; i < cap; ++i) c[i] -= hj * cn[k][i];
          is_new = true;
          break;
        }
      if (!is_new) c[j] -= hj;
    }
    for (auto& v : c) v /= wn;
    for (int64_t i = 0; i < cap; ++i) y[i] += alpha * c[i];
    cn.push_back(std::move(c));
    slots.push_back(slot);
  }
  bool pending(int m) const {            // anything for a flush over m columns to do?
    bool any = knew() > 0;
    for (int j = 0; j < m && !any; ++j) any = y[j] != 0.0;
    return any;
  }
  // what launch_gcr_flush reads over m columns: y [m], then cn as kw = gcr_flush_width(knew) columns of m (unused ones zero)
  std::vector<double> pack(int m, int kw) const {
    std::vector<double> out((size_t)m * (kw + 1), 0.0);
    std::copy(y.begin(), y.begin() + m, out.begin());
    for (int k = 0; k < knew(); ++k) std::copy(cn[k].begin(), cn[k].begin() + m, out.begin() + (size_t)m * (k + 1));
    return out;
  }
  void clear() {
    std::fill(y.begin(), y.end(), 0.0);
    cn.clear();
    slots.clear();
  }
};

// ---- policies ----------------------------------------------------------------------------------------------------------------
// |w'| <= reorth |w| after a Gram-Schmidt pass asks for a second one.
// FP32 storage: a cycle never has to reach below 1e-5 of its start, and the restart from the true residual absorbs
// what a single pass leaves behind, so only a cancellation beyond 100x asks for the second pass
inline double gcr_reorth_threshold(bool f32, bool part, double rtol_floor, double forced) {
  double reorth = f32 ? 0.01 : std::min(0.5, std::max(0.01, 1.0 / (rtol_floor * 9e10)));
  if (part && !f32) reorth = std::max(reorth, 0.1);      // partitioned FP64 basis: |w'|^2 is not measured in the first pass (see gcr_orthogonalise)
  if (forced > 0.0) reorth = forced;
  return reorth;
}

// What one pass leaves of span(Q) in w' is (non-orthonormality of Q) x (cancellation |w| / |w'|), and that is the new
// column's own error against the kept ones: with cancellations of 10 - 200 on most iterations a loose criterion lets
// Q^T Q - I grow by that factor per column (measured on the avf problem, FP64 basis, second pass only beyond 100x:
// 1.5e-4, 4e-3, then q_217 . q_221 = 1.0 - duplicate columns, |r| flat for 40 iterations at a time).  The pass itself
// tells: |w'|^2 measured by the update kernel against |w|^2 - |h|^2, which differ by h^T (Q^T Q - I) h; their relative
// difference over the cancellation estimates the error the new column would carry, and a second pass is made when
// that exceeds the floor of the basis (FP64: 1e-9; FP32 columns are orthonormal to 6e-8 by storage: 3e-7 - scanned on the
// 100-step run of the bench problem: 1e-5 and 1e-6 leave two fall-backs from the FP32 basis late in a Jacobian's life,
// 3e-7 none, 13.1 against 12.2 - 12.35 Newton-it/s; the 20-step bench pays 0.6 %).
// h: the m coefficients of the pass, w2 = |w|^2 before it, wn2 = |w'|^2 as measured after it
inline bool gcr_orth_lost(const double* h, int m, double w2, double wn2, double floor) {
  if (!(wn2 > 0.0 && w2 > 0.0)) return false;
  double hsq = 0.0;
  for (int j = 0; j < m; ++j) hsq += h[j] * h[j];
  const double disc = std::fabs(wn2 - (w2 - hsq)) / wn2;
  const double canc = std::sqrt(w2 / wn2);
  return disc / canc > floor;
}

enum class GcrEnd { go = 0, stagnated = 1, stalled = 2 };
// Whether a cycle goes on, asked before every iteration.  since_gain: iterations since |r| last fell by 10 %.
inline GcrEnd gcr_cycle_end(int since_gain, bool f32, double rnorm, double target, double r_entry, bool store_full) {
  // attainable accuracy: near round-off (a tolerance of 1e-11 on a system with the 1e7 penalty) the recurrence can hover just
  // above the target for thousands of iterations; 40 iterations without a 10 % gain within a factor 100 of the target (FP32
  // basis: anywhere - the restart from the true residual is harmless) end the cycle and solve_gcr decides
  if (since_gain >= 40 && (f32 || rnorm <= 100.0 * target)) return GcrEnd::stagnated;
  // FP32 basis, four decades below the residual the cycle was entered with and six iterations without a 10 % gain: this is
  // the floor of the FP32 columns, not a plateau - the new q are orthogonal to the kept ones to 1e-7 times the cancellation,
  // r has collected that much of span(Q), and directions made orthogonal to Q cannot remove it.  Ending the cycle costs the
  // verdict's product and a projection, which removes it at once (48 k-tet mesh: |r| crawled from 6.05e-8 to 6.01e-8 in 37
  // iterations, and the projection that followed took it to a third of the target without a single new direction).
  if (f32 && since_gain >= 6 && rnorm <= 1e-4 * r_entry) return GcrEnd::stagnated;
  // Far from the target, the store full (the oldest directions kept, a ring of 64 rotating) and no 10 % gain in two turns
  // of the ring: the TRUNCATED recurrence is stuck where the full one would sit out the plateau - seen late in a Jacobian's
  // life on the known-answer case driven to round-off, |r| flat to four digits for 3 700 iterations.  solve_gcr drops the
  // kept directions and restarts from the true residual with room for a full recurrence again.  (Not applied while the
  // store still grows: plateaus of 100+ iterations are normal on these systems, and a restart inside one loses the space
  // that is about to end it.)
  if (since_gain >= 128 && store_full) return GcrEnd::stalled;
  return GcrEnd::go;
}

// What a solve knows when a cycle has ended and its answer is to be judged
struct GcrVerdictIn {
  double rtol, rnorm, bnorm;           // tolerance of the solve, recurrence residual, |b|
  int cyc, cycle_its;                  // index of the cycle in this solve, its iterations
  bool stagnated, stalled;             // how it ended
  bool store_full;
};

// FP64 basis: is the verdict of b - A x due on this cycle's answer?
// When the verdict is taken: always for tight answers (below 1e-8), after anything that has shown the pairs at risk - a
// fall-back from the FP32 basis in this Jacobian's life, a full (rotating) store, a cycle of more than 64 iterations, a
// stalled or stagnated cycle, an earlier verdict of this store that differed from its recurrence by more than a tenth
// of the tolerance - and on the first cycle's answer otherwise NOT: with a fresh Jacobian, a growing store and loose
// tolerances (the all-FP64-storage production runs: 1e-5 .. 1e-2) the pairs hold to 1e-9 (measured), the FP64
// operator is the one the iterations ran on, and the product is 2.7 % of such a run.
inline bool gcr_verdict_due(const GcrVerdictIn& v, bool fell_back, bool suspect) {
  return v.rtol < 1e-8 || fell_back || v.store_full || v.cycle_its > 64 || v.stalled || v.stagnated || suspect || v.cyc > 0 ||
         v.rnorm > v.rtol * v.bnorm;
}

// FP32 basis: may the verdict of b - A x be skipped on this cycle's answer?
// A loose answer (the later Newton iterations of a step ask for 1e-3 .. 1e-2; 38 of the bench's 58 solves, 2.65 ms of FP64
// product each): recurrence and truth agree to three digits and better there (every FP32 cycle of the bench and of the avf
// runs, once the kept columns stay orthonormal - the first attempt at this skip met a solve that reported 1e-2 with a
// true residual of 1.7 |b|: duplicate columns, see the orthogonality criterion gcr_orth_lost), and the next thing that
// happens is Newton's assembly of the FP64 residual from the updated state, the judge of the step either way.  Skipped
// only while the LAST VERIFIED cycle on this store found recurrence and truth closer than 1 % of what is asked now, the
// new directions all sat in the exact FP64 window and nothing stagnated.
// Only inside fsi_newton_solve (in_newton): there the FP64 residual assembled from the updated state follows and judges the
// step.  A direct fsi_solve caller has no such judge, so its answers always get the FP64 verdict and `relres`
// is the true residual; when verdicts_skipped counts up, the FsiNewtonIter.lin_relres of that iteration is the recurrence value.
inline bool gcr_verdict_skippable(const GcrVerdictIn& v, bool in_newton, bool final_cycle, double skip_rtol, double last_drift) {
  return in_newton && final_cycle && v.rtol >= skip_rtol && v.rnorm <= v.rtol * v.bnorm && v.cycle_its <= GCR_WINDOW && !v.stagnated &&
         last_drift >= 0.0 && last_drift <= 0.01 * v.rtol;
}

// adaptive solve: start where the last check under this Jacobian says the unscaled criterion will be met (a re-entered cycle
// costs a projection on the kept space and a flush - three passes over the store - so guessing right the first time matters)
inline double gcr_adaptive_start(double rtol, double utol, double utol_ratio, double rtol_floor) {
  if (utol > 0.0 && utol_ratio > 0.0 && rtol > rtol_floor) return std::max(rtol_floor, std::min(rtol, 0.7 * utol / utol_ratio));
  return rtol;
}
// ... and the next tolerance when the unscaled residual ru still exceeds utol * b_unscaled
inline double gcr_adaptive_tighten(double rtol, double utol, double b_unscaled, double ru, double rtol_floor) {
  const double want = 0.5 * utol * b_unscaled / ru;              // aim a factor two below
  return std::max(rtol_floor, rtol * std::min(0.5, std::max(0.02, want)));
}

// Storage of Q for this Jacobian's lifetime, decided by the first solve after the refresh: FP32 (half the dominant
// stream, exact FP64 window for the directions of the current cycle, restart from the true residual) when the accuracy
// that may be asked for during the lifetime leaves room for it.  Inside fsi_newton_solve that is the floor of the
// forcing term at the largest right-hand side seen so far (tol_hint); the inexact-Newton tolerances of a production run
// qualify (5e-7 on the bench), the parity tests that drive Newton to round-off keep FP64.
inline bool gcr_basis_fp32(double tol_hint, double rtol, double fp32_floor) {
  const double lowest = tol_hint > 0.0 ? std::min(tol_hint, rtol) : rtol;
  return lowest > fp32_floor;
}

}  // namespace fsi
