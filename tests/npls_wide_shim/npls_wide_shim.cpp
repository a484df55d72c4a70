// npls_wide_shim.cpp — TEST INFRASTRUCTURE: Ops::npls_contract_wide and Ops::npls_slice_inner_wide of a back end on
// host arrays, with the route log of the call (tests/npls_cv_cases.py). Linked against libppals.so it reaches the HIP
// kernels as compiled there, linked against the host stand-in the defaults of ops.h; no HIP code and no HIP calls
// here: every device action goes through the Ops.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "backend.h"

using namespace ppals;

namespace {
Ops *g_ops = nullptr;
std::string g_err;

Ops &ops() {
  if (!g_ops) g_ops = backend_make_ops(0);
  g_ops->bind();
  return *g_ops;
}
}  // namespace

extern "C" {
const char *npls_wide_shim_error() { return g_err.c_str(); }

// op 0: Z[l,t,c] = sum_i X[l,i,t] in[i,c] (in: I x C, out: L T C doubles); op 1: S[i,c] = sum_{l,t} X[l,i,t] in[l,t,c]
// (in: L T C, out: I x C). X: L I T elements of the storage type dt (F32 = 0, F64 = 1, BF16 = 3), uploaded as they are.
// out comes with `guard` doubles in front and behind, prefilled by the caller, uploaded and downloaded whole. route:
// the newline-joined route tags of the call. Returns 0, or -1 with npls_wide_shim_error().
int npls_wide_shim_run(int op, int dt, const void *X, int64_t L, int64_t I, int64_t T, const double *in, int C,
                       double *out, int64_t guard, char *route, int route_len) {
  try {
    Ops &o = ops();
    const size_t nX = (size_t)(L * I * T) * dtype_size(dt);
    const size_t nin = sizeof(double) * (size_t)((op == 0 ? I : L * T) * C);
    const size_t nout = sizeof(double) * (size_t)(2 * guard + (op == 0 ? L * T : I) * C);
    void *dX = o.alloc(nX);
    double *din = (double *)o.alloc(nin), *dout = (double *)o.alloc(nout);
    o.h2d(dX, X, nX);
    o.h2d(din, in, nin);
    o.h2d(dout, out, nout);
    std::vector<std::string> log;
    o.route_log = &log;
    if (op == 0)
      o.npls_contract_wide(dX, dt, L, I, T, din, C, dout + guard);
    else
      o.npls_slice_inner_wide(dX, dt, L, I, T, din, C, dout + guard);
    o.route_log = nullptr;
    o.d2h(out, dout, nout);
    o.free(dX);
    o.free(din);
    o.free(dout);
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

void npls_wide_shim_close() {
  try {
    delete g_ops;
  } catch (...) {
  }
  g_ops = nullptr;
}
}
