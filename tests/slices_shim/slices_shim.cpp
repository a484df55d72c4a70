// slices_shim.cpp — TEST INFRASTRUCTURE: Ops::residual_slices of the product's back end on host arrays, with
// the route log of the call (tests/test_gpu_slices_routes.py). Linked against libppals.so, it reaches the HIP
// kernels as compiled there; no HIP code and no HIP calls here: every device action goes through the Ops.
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
const char *slices_shim_error() { return g_err.c_str(); }
// V: M x K elements of storage type dt as stored (first index fastest); Q: M x R, P: K x R, column-major fp64.
// misalign != 0: the tensor starts 8 bytes into its allocation (an unaligned shard). Outputs on the host;
// route: the newline-joined route tags of the call. Returns 0, or -1 with slices_shim_error().
int slices_shim_run(int dt, int64_t M, int64_t K, int R, const void *V, const double *Q, const double *P,
                    uint64_t cap, int misalign, double *rowsq, double *colsq, double *total, char *route,
                    int route_len) {
  try {
    if (!g_ops) g_ops = backend_make_ops(0);
    Ops &o = *g_ops;
    o.bind();
    const size_t vb = (size_t)M * K * dtype_size(dt), off = misalign ? 8 : 0;
    char *dV = (char *)o.alloc(vb + off);
    double *dQ = (double *)o.alloc(sizeof(double) * M * R), *dP = (double *)o.alloc(sizeof(double) * K * R);
    double *dr = (double *)o.alloc(sizeof(double) * (M + K + 1)), *dc = dr + M, *dt_ = dc + K;
    o.h2d(dV + off, V, vb);
    o.h2d(dQ, Q, sizeof(double) * M * R);
    o.h2d(dP, P, sizeof(double) * K * R);
    std::vector<std::string> log;
    o.route_log = &log;
    void *work = nullptr;
    size_t work_bytes = 0;
    o.residual_slices(dV + off, dt, M, K, dQ, dP, R, dr, dc, dt_, (size_t)cap, work, work_bytes);
    o.route_log = nullptr;
    o.d2h(rowsq, dr, sizeof(double) * M);
    o.d2h(colsq, dc, sizeof(double) * K);
    o.d2h(total, dt_, sizeof(double));
    for (void *p : {(void *)dV, (void *)dQ, (void *)dP, (void *)dr, work}) o.free(p);
    std::string joined;
    for (const std::string &t : log) joined += (joined.empty() ? "" : "\n") + t;
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
void slices_shim_close() {
  try {
    delete g_ops;
  } catch (...) {
  }
  g_ops = nullptr;
}
}
