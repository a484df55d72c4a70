// run_report.h — what the CP and Tucker ALS drivers report about a run, in the reference's formats
// (rank-0 cout / printf and CSV of als_CP.cxx and als_Tucker.cxx): the CSV stream, the run clock,
// the per-iteration row, pp_bench's timings and the closing lines; and the per-mode norms both
// engines' restart tests read. Host only, HIP-free.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "engine.h"

namespace ppals {

inline double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

class RunReport {
 public:
  // Rank 0 opens the CSV (appends with o.csv_append) and, unless o.bench, writes its header; then
  // the clock starts. metric: the row's convergence measure, "gradnorm" (CP) or "diffnorm" (Tucker).
  RunReport(const CpOpts &o, bool rank0, int64_t dim, const char *metric)
      : talk_(rank0 && o.verbose), dim_(dim), tol_(o.tol), metric_(metric) {
    if (rank0 && !o.csv_path.empty()) {
      csv_.open(o.csv_path, o.csv_append ? std::ios::app : std::ios::out);
      if (!o.bench) csv_ << "[dim],[iter],[" << metric << "],[tol],[pp_update],[diffV],[dtime]\n";
    }
    st_time_ = now();
  }

  double elapsed() const { return now() - st_time_; }
  // runs f with the clock stopped: a measurement does not count as run time (st_time += ...)
  template <class F>
  void off_clock(F &&f) {
    const double t = now();
    f();
    st_time_ += now() - t;
  }

  // the print block's row: console at precision 13 (which stays set), CSV at the default 6 and a
  // blank CSV line after every 100th iteration (als_CP.cxx:166-213)
  void row(int iter, double norm, int pp_flag, double diffV) {
    const double dtime = elapsed();
    if (talk_) {
      std::cout.precision(13);
      std::cout << "  [dim]=  " << dim_ << "  [iter]=  " << iter << "  [" << metric_ << "]  "
                << norm << "  [tol]  " << tol_ << "  [pp_update]  " << pp_flag << "  [diffV]  "
                << diffV << "  [dtime]  " << dtime << "\n";
    }
    if (csv_.is_open()) {
      csv_ << dim_ << "," << iter << "," << norm << "," << tol_ << "," << pp_flag << "," << diffV
           << "," << dtime << "\n";
      if (iter % 100 == 0 && iter != 0) csv_ << std::endl;
    }
  }
  // pp_bench, exact phase (als_CP.cxx:203-209): the time of the sweeps since the start
  void dt_bench_time() {
    const double dtime = elapsed();
    if (talk_) std::cout << "  [dimension tree step time]  " << dtime << "\n";
    if (csv_.is_open()) csv_ << "[DTtime]" << "," << dtime << "\n";
  }
  // pp_bench, PP phase (als_CP.cxx:735-748): a report before maxiter restarts the clock; the one at
  // maxiter writes its own time ([PPsecond]) and that plus the time before the last restart in the
  // same phase ([PPfirst]; every PP phase starts it at 0, als_CP.cxx:627)
  void start_pp_phase() { pp_first_ = 0; }
  void pp_bench_time(int iter, int maxiter) {
    const double dtime = elapsed();
    if (iter != maxiter) {
      pp_first_ = dtime;
      st_time_ = now();
      return;
    }
    pp_first_ += dtime;
    if (talk_) {
      std::cout << "  [PP first time]  " << pp_first_ << "\n";
      std::cout << "  [PP second time]  " << dtime << "\n";
    }
    if (csv_.is_open()) {
      csv_ << "  [PPfirst]  " << "," << pp_first_ << "\n";
      csv_ << "  [PPsecond]  " << "," << dtime << "\n";
    }
  }

  void dot(int iter) const {
    if (iter % 10 == 0 && talk_) printf(".");
  }
  void starts(const char *phase, int iter) const {
    if (talk_) printf("%s starts from %d\n", phase, iter);
  }
  // what: "proj-grad" (CP DT), "grad" (CP PP) or "Diff" (Tucker)
  void finish(int iter, const char *what, double norm) const {
    if (!talk_) return;
    printf("\nIter = %d Final %s norm %E \n", iter, what, norm);
    printf("tf took %lf seconds\n", elapsed());
  }

 private:
  const bool talk_;
  const int64_t dim_;
  const double tol_;
  const char *const metric_;
  std::ofstream csv_;
  double st_time_ = 0, pp_first_ = 0;
};

// ||dW_i|| and ||W_i|| of every mode, from the device's 2N sums of squares ||dW_0||^2, ||W_0||^2, ...
struct ModeNorms {
  int n;
  double d[MAX_ORDER], w[MAX_ORDER];
  ModeNorms(Ops &ops, const double *sums, int N) : n(N) {
    double h[2 * MAX_ORDER];
    ops.d2h(h, sums, sizeof(double) * 2 * N);
    for (int i = 0; i < N; i++) {
      d[i] = std::sqrt(h[2 * i]);
      w[i] = std::sqrt(h[2 * i + 1]);
    }
  }
  // modes whose |d/w| lies above tol (above) or below it
  int count(double tol, bool above) const {
    int c = 0;
    for (int i = 0; i < n; i++) {
      const double r = std::fabs(d[i] / w[i]);
      c += above ? r > tol : r < tol;
    }
    return c;
  }
};

}  // namespace ppals
