// The coefficient schedule of a Chebyshev chain and the loop that runs one.  A sweep does  x += d_in;  r -= A d_in;
// d_out = c1 d_in + c2 B^-1 r;  the first direction is  d_0 = init() B^-1 r.  Plain C++: the block preconditioner
// (fsi_precond.hip) and the test shim read the same arithmetic, in double; callers cast to float where their kernel takes one.
#pragma once

namespace fsi {

struct ChebSchedule {
  double lmax, lmin, th, de, sig, rho;
  bool fourth;
  int i = 1;                                 // 4th kind: index of the next direction
  // The classic three-term recurrence on [lmax / kappa, lmax].  fourth: Chebyshev polynomials of the 4th kind instead (Lottes
  // 2022: the smoother that minimises the two-level bound for a given degree; needs lmax only):  d_0 = 4/(3 lmax) B^-1 r,
  // d_i = (2i-1)/(2i+3) d_{i-1} + (8i+4)/((2i+3) lmax) B^-1 r_i
  ChebSchedule(double lmax_, double kappa, bool fourth_ = false)
      : lmax(lmax_), lmin(lmax / kappa), th(0.5 * (lmax + lmin)), de(0.5 * (lmax - lmin)), sig(th / de), rho(1.0 / sig), fourth(fourth_) {}
  double init() const { return fourth ? 4.0 / (3.0 * lmax) : 1.0 / th; }
  void next(double* c1, double* c2) {
    if (fourth) {
      *c1 = (2.0 * i - 1.0) / (2.0 * i + 3.0);
      *c2 = (8.0 * i + 4.0) / ((2.0 * i + 3.0) * lmax);
      i += 1;
      return;
    }
    const double rn = 1.0 / (2.0 * sig - rho);
    *c1 = rn * rho;
    *c2 = 2.0 * rn / de;
    rho = rn;
  }
  void restart() { rho = 1.0 / sig; i = 1; }      // the tail chain of a two-level cycle starts the recurrence again
};

struct ChainRun {
  int launched;         // sweeps launched
  bool d_left;          // the last sweep was not launched: the chain's consumer takes x and the current direction and adds them
};

// The last sweep of a Chebyshev chain is not launched (drop).  What follows a chain reads x alone: the last product feeds only
// an r and a d that nobody reads.  The chain's consumer takes x and the current direction and forms x + d itself, the same
// addition in the same precision (fsi_block.hip, k_unpad_from_f32), so an application's output keeps its bits.
// Runs `count` sweeps of a chain, sweep(k, c1, c2) launching the k-th.  restart: the chain is the tail of a two-level cycle -
// its first sweep takes the prolonged coarse correction as its direction (x += P x_c, r -= A P x_c) and starts the
// recurrence again, d_out = init() B^-1 r; the post-smoothing sweeps follow.
template <class Sweep>
inline ChainRun run_chain(ChebSchedule& gen, int count, bool drop, Sweep&& sweep, bool restart = false) {
  const int launched = (count > 0 && drop) ? count - 1 : count;
  for (int k = 0; k < launched; ++k) {
    double c1 = 0.0, c2 = gen.init();
    if (restart && k == 0) gen.restart();
    else gen.next(&c1, &c2);
    sweep(k, c1, c2);
  }
  return ChainRun{launched, launched < count};
}

}  // namespace fsi
