// dc_chain.hpp -- the DC fallback chain of the reference (_dc_solve_with_fallbacks, solve.jl:871-929) as host-only policy, PER
// INSTANCE: sweep points are independent circuits (sweeps.jl:696-703), so an instance leaves the chain at the first stage that
// converges for it and its solution is never touched again; only the instances still unsolved take part in the later stages, each
// on its own homotopy ladder.
//   stage 0  PCNR Newton from the caller's start point (solve.jl:599-698)  -- or plain Newton when use_pcnr is off
//   stage 1  plain Newton from the caller's start point (solve.jl:899-903); only with PCNR on and limit variables present
//   stage 2  gshunt stepping from zero: 1e-3, /10 ... 1e-12, then the target; a failed rung restores the last solution
//            and takes the square root of the factor until it is <= 1.5 (solve.jl:720-783)
//   stage 3  source stepping from zero: srcFact 0, +0.1 ... 1; a failed rung halves the raise (solve.jl:805-850)
// No HIP, no handle: the chain reaches the device through one runner (DCRun), which cadnip_dc_run (driver.hip) supplies and
// tests/test_dc_chain_cpu.py replaces by the oracle's Newton functions.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <memory>
#include <vector>

namespace cadnip {

// one Newton run of one instance, as cadnip_dc_log_* reports it
struct DCLogEntry { int inst, stage; double value; int ok; long long iters; };

struct DCChainOpts {
  int use_pcnr, cold_start, fused, use_stepping;   // cold_start 2 (CADNIP_DC_COLD_ZERO) without a mask: cold from the all-zero state, `u` is output only
                                                   // (nothing of it is read); with a mask it is 1 and u is read -- masked rows come back untouched
  bool has_limits;             // the circuit has limit variables (stage 1 exists only then)
  double gshunt, srcFact;      // the spec's values: what every instance outside a ladder is stamped with, and the gshunt ladder's target
  const int* participate;      // [B] or null = everyone; 0 = the instance sits the call out (no run, u untouched, converged 0)
};

// One Newton run of the batch, as the chain asks the runner for it: `int runner(const DCRun&)`, 0 = done, anything else ends the
// chain with that code.  The runner solves the instances with part[i] != 0 -- the chain never asks with nobody in `part`, nor for
// an instance that has finished -- each from u[i] with its own (gshunt[i], srcFact[i]), and fills in, in this order, status,
// the end states at dest() and iters.  Rows of instances outside `part` are never read by the chain.
struct DCRun {
  int stage, use_pcnr, cold_start, fused;
  const int* part;                    // [B]
  const double* u;                    // [B][n] start states (the caller's array on the first run); null = all zero (the first run of a
                                      // zero start, cold_start 2): the runner makes its own zeros, nothing is handed over
  const double *gshunt, *srcFact;     // [B]
  int* status;                        // [B] 1 = converged
  long long* iters;                   // [B] Newton solves
  double *R, *R_direct;               // [B][n] end states; R_direct: non-null on the first run of an unmasked batch (the caller's array)
  int B;
  // where the end states go once `status` is known: straight to the caller when the first run solved everybody
  double* dest() const {
    if (!R_direct) return R;
    for (int i = 0; i < B; ++i) if (status[i] != 1) return R;
    return R_direct;
  }
};

struct DCChainResult {
  long long iters = 0;     // Newton solves of all runs
  int n_failed = 0;        // participating instances no stage solved
  bool direct = false;     // the first run solved everybody: the runner's device state is the result, `u` has it already
};

namespace dc_chain_detail {

enum Next { AGAIN, SOLVED, GAVE_UP };

// The two rung rules.  value(): the homotopy term of the next run; digest(): what the run's verdict does to the ladder.
struct GshuntRule {                            // solve.jl:720-783
  double target, gfloor;
  struct State { double g = 1e-3, factor = 10.0; int steps = 0; bool finalizing = false; };
  explicit GshuntRule(double t) : target(t), gfloor(std::fmax(t, 1e-12)) {}
  double value(const State& s) const { return s.finalizing ? target : s.g; }
  Next digest(State& s, bool ok) const {
    if (s.finalizing) return ok ? SOLVED : GAVE_UP;       // the solve at the exact target ends the ladder either way
    ++s.steps;
    if (ok) {
      if (s.g <= gfloor) {
        if (s.g == target) return SOLVED;
        s.finalizing = true;
        return AGAIN;
      }
      s.g /= s.factor;
      if (s.g < gfloor) s.g = gfloor;
    } else {
      if (s.factor <= 1.5) return GAVE_UP;                // cannot make progress
      s.factor = std::sqrt(s.factor);
    }
    return s.steps >= 20 ? GAVE_UP : AGAIN;               // max_steps
  }
};

struct SourceRule {                            // solve.jl:805-850
  struct State { double src = 0.0, conv = 0.0, raise = 0.1; int steps = 0; };
  double value(const State& s) const { return s.src; }
  Next digest(State& s, bool ok) const {
    ++s.steps;
    if (ok) {
      s.conv = s.src;
      if (s.src >= 1.0) return SOLVED;
      s.src = std::fmin(s.src + s.raise, 1.0);
    } else {
      if (s.src - s.conv < 1e-6) return GAVE_UP;
      s.raise /= 2.0;
      s.src = s.conv + s.raise;
    }
    return s.steps >= 50 ? GAVE_UP : AGAIN;               // max_steps
  }
};

// one instance's walk through a stepping stage.  `u` is its last solution (zero before the first): the start of its next run, and
// what the instance is left with when the ladder gives up
template <class Rule> struct Ladder { typename Rule::State s; bool over = false; std::vector<double> u; };

}  // namespace dc_chain_detail

// Walks the batch through the chain.  u [B][n]: start states in, final states out (a solved instance's solution; an unsolved
// one's state as its last ladder left it; a masked one's untouched).  converged [B] (may be null).  Every run of every instance
// is appended to `log` in execution order.  Returns 0, or the runner's code as soon as a run fails (u and converged are then
// not written).
template <class Runner>
int dc_chain(const DCChainOpts& o, int B_, int n_, double* u, int* converged, Runner&& runner, std::vector<DCLogEntry>& log, DCChainResult& res) {
  using namespace dc_chain_detail;
  const size_t B = (size_t)B_, n = (size_t)n_;
  res = DCChainResult();
  // per-instance start state of the next run / states after the last run.  `start` and `U` are built only when the first run leaves
  // someone unsolved: the usual case -- everybody converges in stage 0 -- hands the caller's array to the runner and gets it back filled
  std::vector<double> start, U;
  // R, the end states of a run that does not go straight to the caller, is allocated and NOT initialised: in the usual case no run's
  // dest() is R, and zero-filling B * n doubles on fresh pages for nothing was a measurable part of the call.  No uninitialised word
  // is ever read: R is read in two places only, take_all and the ladders' digest loop in `stepping`, both after run() has returned 0
  // and both for rows with part[i] != 0 alone -- the very rows the runner of that run has just filled (DCRun: the runner writes the end
  // states of the instances in `part` to dest(), which is R whenever res.direct is false; after a direct run R is not looked at).
  // CADNIP_DC_CHAIN_POISON (tests) fills R with NaN instead, so that a read of a row no runner wrote would show in the results
  const std::unique_ptr<double[]> R_store(new double[B * n]);
  double* const R = R_store.get();
#ifdef CADNIP_DC_CHAIN_POISON
  std::fill(R, R + B * n, std::numeric_limits<double>::quiet_NaN());
#endif
  // a zero start: nothing of `u` is read, the first run starts from the runner's own zeros (DCRun::u null)
  const bool zero_start = o.cold_start == 2 && !o.participate;
  const int cold_start = o.cold_start == 2 && !zero_start ? 1 : o.cold_start;
  std::vector<int> fin(B, 0), status(B), part(B, 1);
  std::vector<long long> iters(B);
  std::vector<double> gsh(B, o.gshunt), sfc(B, o.srcFact);
  auto masked = [&](size_t i) { return o.participate && !o.participate[i]; };
  for (size_t i = 0; i < B; ++i) if (masked(i)) { part[i] = 0; fin[i] = 1; }   // (fin: no stage picks them up)
  auto n_open = [&]() { int k = 0; for (size_t i = 0; i < B; ++i) k += !fin[i]; return k; };
  auto row = [&](std::vector<double>& v, size_t i) { return v.begin() + i * n; };
  auto Rrow = [&](size_t i) { return R + i * n; };
  // one Newton run of the instances in `part`; rung: the term that is stepped ([B], null: none)
  auto run = [&](int stage, int use_pcnr, int cold_start, int fused, const double* from, const double* rung, double* R_direct) -> int {
    const DCRun r{stage, use_pcnr, cold_start, fused, part.data(), from, gsh.data(), sfc.data(), status.data(), iters.data(), R, R_direct, B_};
    if (int rc = runner(r)) return rc;
    res.direct = R_direct && r.dest() == R_direct;
    for (size_t i = 0; i < B; ++i)
      if (part[i]) { res.iters += iters[i]; log.push_back({(int)i, stage, rung ? rung[i] : 0.0, status[i] == 1 ? 1 : 0, iters[i]}); }
    return 0;
  };
  // the instances of the run leave it with its end state, solved or not
  auto take_all = [&]() { for (size_t i = 0; i < B; ++i) if (part[i]) { std::copy(Rrow(i), Rrow(i + 1), row(U, i)); if (status[i] == 1) fin[i] = 1; } };
  // stages 2 and 3: one ladder per open instance, all ladders advanced by one run per round
  auto stepping = [&](int stage, auto rule, std::vector<double>& term, double spec_value) -> int {
    std::vector<Ladder<decltype(rule)>> L(B);
    for (size_t i = 0; i < B; ++i) { L[i].over = fin[i]; if (!fin[i]) L[i].u.assign(n, 0.0); }
    for (;;) {
      int k = 0;
      for (size_t i = 0; i < B; ++i) {
        part[i] = !L[i].over;
        term[i] = part[i] ? rule.value(L[i].s) : spec_value;
        if (part[i]) { ++k; std::copy(L[i].u.begin(), L[i].u.end(), row(U, i)); }
      }
      if (!k) return 0;                        // (every term is back at the spec's value)
      if (int rc = run(stage, 0, 0, 0, U.data(), term.data(), nullptr)) return rc;
      for (size_t i = 0; i < B; ++i) {
        if (!part[i]) continue;
        const bool ok = status[i] == 1;
        if (ok) L[i].u.assign(Rrow(i), Rrow(i + 1));
        const Next next = rule.digest(L[i].s, ok);
        if (next == AGAIN) continue;
        L[i].over = true;
        fin[i] = next == SOLVED;
        std::copy(L[i].u.begin(), L[i].u.end(), row(U, i));
      }
    }
  };
  // ---- stage 0: PCNR (or plain Newton) from the caller's start point
  if (n_open())
    if (int rc = run(0, o.use_pcnr, cold_start, o.fused, zero_start ? nullptr : u, nullptr, o.participate ? nullptr : u)) return rc;
  if (res.direct) {
    if (converged) std::fill(converged, converged + B, 1);
    return 0;
  }
  if (zero_start) start.assign(B * n, 0.0);   // (u holds whatever the caller allocated; every row of it is overwritten below)
  else start.assign(u, u + B * n);
  U = start;
  take_all();
  // ---- stage 1: plain Newton from the caller's start point, for those PCNR did not solve
  if (n_open() && o.use_pcnr && o.has_limits) {
    for (size_t i = 0; i < B; ++i) { part[i] = !fin[i]; if (part[i]) std::copy(row(start, i), row(start, i + 1), row(U, i)); }
    if (int rc = run(1, 0, 0, 0, U.data(), nullptr, nullptr)) return rc;
    take_all();
  }
  // ---- stage 2: gshunt stepping; stage 3: source stepping for the rest
  if (n_open() && o.use_stepping)
    if (int rc = stepping(2, GshuntRule(o.gshunt), gsh, o.gshunt)) return rc;
  if (n_open() && o.use_stepping)
    if (int rc = stepping(3, SourceRule(), sfc, o.srcFact)) return rc;
  res.n_failed = n_open();
  std::copy(U.begin(), U.end(), u);
  if (converged) for (size_t i = 0; i < B; ++i) converged[i] = masked(i) ? 0 : fin[i];
  return 0;
}

}  // namespace cadnip
