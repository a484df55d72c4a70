// shape_shim.cpp — TEST INFRASTRUCTURE: Ops::cp_mode_update_shape_ragged of a back end on host arrays, with the
// route log of the call (tests/shape_cases.py). Linked against libppals.so it reaches the HIP kernels as compiled
// there, linked against the host stand-in the ops.h default; no HIP code and no HIP calls here: every device
// action goes through the Ops.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "backend.h"

using namespace ppals;

namespace {
Ops *g_ops = nullptr;
std::string g_err;
}  // namespace

extern "C" {
const char *shape_shim_error() { return g_err.c_str(); }
// `nstarts` starts of the ranks `ranks`, C columns and Q = sum R_b^2 in all. Gall: the N Grams of every start
// (N * Q doubles, start b's at N sq_b; the one of `mode` is overwritten). M: ldm x C. W, grad: `guard` doubles,
// then ld x C, then `guard` doubles — handed to the op as they are, guards and the rows behind `rows` included,
// and copied back whole, so the caller sees every double the op could have touched. gradsq: nstarts. S: Q, or
// NULL for a call that does not ask for the systems. shape: PPALS_SHAPE_UNIMODAL, _INCREASING or _DECREASING.
// route: the newline-joined route tags of the call.
// Returns 0, or -1 with shape_shim_error().
int shape_shim_run(int N, int mode, int nstarts, const int *ranks, double lambda, int64_t rows, int64_t ldm,
                   int64_t ldw, int64_t ldg, int64_t guard, double *Gall, const double *M, double *W, double *grad,
                   double *gradsq, double *S, int shape, char *route, int route_len) {
  try {
    if (!g_ops) g_ops = backend_make_ops(0);
    Ops &o = *g_ops;
    o.bind();
    StartTable t;
    t.nstarts = nstarts;
    for (int b = 0; b < nstarts; b++) {
      t.col[b + 1] = t.col[b] + ranks[b];
      t.sq[b + 1] = t.sq[b] + ranks[b] * ranks[b];
    }
    const size_t C = (size_t)t.col[nstarts], Q = (size_t)t.sq[nstarts];
    const size_t nG = sizeof(double) * N * Q, nM = sizeof(double) * ldm * C;
    const size_t nW = sizeof(double) * (2 * guard + ldw * C), nGr = sizeof(double) * (2 * guard + ldg * C);
    double *dG = (double *)o.alloc(nG), *dM = (double *)o.alloc(nM), *dW = (double *)o.alloc(nW);
    double *dGr = (double *)o.alloc(nGr), *dsq = (double *)o.alloc(sizeof(double) * nstarts);
    double *dS = S ? (double *)o.alloc(sizeof(double) * Q) : nullptr;
    o.h2d(dG, Gall, nG);
    o.h2d(dM, M, nM);
    o.h2d(dW, W, nW);
    o.h2d(dGr, grad, nGr);
    std::vector<std::string> log;
    o.route_log = &log;
    o.cp_mode_update_shape_ragged(dG, N, mode, t, lambda, dM, ldm, dW + guard, ldw, dGr + guard, ldg, rows, dsq, dS,
                                  shape);
    o.route_log = nullptr;
    o.d2h(Gall, dG, nG);
    o.d2h(W, dW, nW);
    o.d2h(grad, dGr, nGr);
    o.d2h(gradsq, dsq, sizeof(double) * nstarts);
    if (S) o.d2h(S, dS, sizeof(double) * Q);
    for (void *p : {(void *)dG, (void *)dM, (void *)dW, (void *)dGr, (void *)dsq, (void *)dS}) o.free(p);
    std::string joined;
    for (const std::string &tag : log) joined += (joined.empty() ? "" : "\n") + tag;
    std::strncpy(route, joined.c_str(), (size_t)route_len - 1);
    route[route_len - 1] = 0;
    return 0;
  } catch (const std::exception &e) {
    g_err = e.what();
  } catch (...) {
    g_err = "unknown exception";
  }
  if (g_ops) g_ops->route_log = nullptr;
  return -1;
}
void shape_shim_close() {
  try {
    delete g_ops;
  } catch (...) {
  }
  g_ops = nullptr;
}
}
