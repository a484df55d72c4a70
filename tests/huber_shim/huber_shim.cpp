// huber_shim.cpp — TEST INFRASTRUCTURE: Ops::model_wls, Ops::model_huber (with and without a weights view) and
// Ops::model_absres_hist of the product's back end on host arrays, with the route log of each call
// (tests/test_gpu_huber_routes.py). Linked against libppals.so, it reaches the HIP kernels as compiled there;
// no HIP code and no HIP calls here: every device action goes through the Ops.
//
// The plan is the simplest one: a box of two modes, A x B, the shard and both views dense with the first index
// fastest, group A = mode 0, group B = mode 1; Q is A x K and P is B x K, column-major fp64.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "backend.h"
#include "device_view.h"

using namespace ppals;

namespace {
Ops *g_ops = nullptr;
std::string g_err;
}  // namespace

extern "C" {
const char *huber_shim_error() { return g_err.c_str(); }
// f32 storage and f32 views. V0, X, H: A x B floats. out: 3 x (A x B) floats, the shard after model_wls, after
// model_huber with the weights and after model_huber without, each from V0; sums: the weighted loss, then (loss,
// clipped) of the two Huber calls; hist: 2 x Ops::ABSRES_BINS counts of the first pass (all keys, the top 11
// bits), with and without the weights; route: the newline-joined route tags of the five calls, in that order.
int huber_shim_run(int64_t A, int64_t B, int K, const float *V0, const float *X, const float *H, const double *Q,
                   const double *P, double c, float *out, double *sums, uint64_t *hist, char *route,
                   int route_len) {
  try {
    if (!g_ops) g_ops = backend_make_ops(0);
    Ops &o = *g_ops;
    o.bind();
    const size_t nb = sizeof(float) * (size_t)(A * B);
    float *dV = (float *)o.alloc(nb), *dX = (float *)o.alloc(nb), *dH = (float *)o.alloc(nb);
    double *dQ = (double *)o.alloc(sizeof(double) * A * K), *dP = (double *)o.alloc(sizeof(double) * B * K);
    double *ds = (double *)o.alloc(sizeof(double) * 2);
    o.h2d(dX, X, nb);
    o.h2d(dH, H, nb);
    o.h2d(dQ, Q, sizeof(double) * A * K);
    o.h2d(dP, P, sizeof(double) * B * K);
    ModelBox bx;
    bx.order = 2;
    bx.len[0] = A;
    bx.len[1] = B;
    bx.vs[0] = bx.rs[0] = 1;
    bx.vs[1] = bx.rs[1] = A;
    ModelPlan mp;
    mp.ga.add(bx, 0);
    mp.gb.add(bx, 1);
    mp.ldq = A;
    mp.pL = B;
    ModelSide ws;
    ws.ga = mp.ga;
    ws.gb = mp.gb;  // (vs: the weights' strides, the data's here)
    std::vector<std::string> log;
    o.route_log = &log;
    for (int call = 0; call < 3; call++) {
      o.h2d(dV, V0, nb);
      if (call == 0)
        o.model_wls(mp, ws, dQ, dP, K, dX, dH, DV_F32, dV, F32, ds, nullptr);
      else
        o.model_huber(mp, call == 1 ? &ws : nullptr, dQ, dP, K, dX, dH, DV_F32, dV, F32, c, ds, nullptr);
      o.d2h(out + (size_t)call * A * B, dV, nb);
      o.d2h(sums + (call == 0 ? 0 : 2 * call - 1), ds, sizeof(double) * (call == 0 ? 1 : 2));
    }
    for (int call = 0; call < 2; call++)
      o.model_absres_hist(mp, call == 0 ? &ws : nullptr, dQ, dP, K, dX, dH, DV_F32, 31, 0u, 20, 2047u,
                          hist + (size_t)call * Ops::ABSRES_BINS, nullptr);
    o.route_log = nullptr;
    for (void *p : {(void *)dV, (void *)dX, (void *)dH, (void *)dQ, (void *)dP, (void *)ds}) o.free(p);
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
void huber_shim_close() {
  try {
    delete g_ops;
  } catch (...) {
  }
  g_ops = nullptr;
}
}
