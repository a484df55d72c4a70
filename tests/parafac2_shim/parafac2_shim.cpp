// parafac2_shim.cpp — TEST INFRASTRUCTURE: Ops::parafac2_step and Ops::parafac2_init of a back end on host
// arrays, with the route log of the call (tests/parafac2_op_cases.py). Linked against libppals.so it reaches the
// HIP kernels as compiled there; no HIP code and no HIP calls here: every device action goes through the Ops.
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

Ops &ops() {
  if (!g_ops) g_ops = backend_make_ops(0);
  g_ops->bind();
  return *g_ops;
}
// a host buffer of `bytes` on the device, as it is
void *upload(Ops &o, const void *h, size_t bytes) {
  void *d = o.alloc(bytes);
  o.h2d(d, h, bytes);
  return d;
}
}  // namespace

extern "C" {
const char *parafac2_shim_error() { return g_err.c_str(); }

// One step on host arrays. X: nX elements of the view type vdt (DV_F32 = 0, DV_F64 = 1), padding included,
// uploaded as it is; element (i, j, k) sits at i + s1 j + s2 k. B (R x R), A (J x R), C (K x R): column-major
// doubles. Q, P (I R K doubles each), T (R R K doubles), status (K ints) and Y (R J K elements of the storage type
// dt, F32 = 0 or F64 = 1) each come with `guard` elements in front and behind, prefilled by the caller: they are
// uploaded whole, the op gets the inner pointers, and each is downloaded whole, so the caller sees every byte
// the op could have touched. out: 3 doubles, or NULL for a call that does not ask for the sums. route: the
// newline-joined route tags of the call. Returns 0, or -1 with parafac2_shim_error().
int parafac2_shim_run(int64_t I, int64_t J, int64_t K, int R, int vdt, int dt, const void *X, int64_t s1, int64_t s2,
                      int64_t nX, const double *B, const double *A, const double *C, double min_ratio, double *Q,
                      double *P, double *T, int *status, void *Y, double *out, int64_t guard, char *route,
                      int route_len) {
  try {
    Ops &o = ops();
    const size_t g = (size_t)guard, ye = dtype_size(dt);
    const size_t nQ = sizeof(double) * (2 * g + (size_t)I * R * K), nT = sizeof(double) * (2 * g + (size_t)R * R * K);
    const size_t nS = sizeof(int) * (2 * g + (size_t)K), nY = ye * (2 * g + (size_t)R * J * K);
    void *dX = upload(o, X, (size_t)nX * dv_elem_size(vdt));
    double *dB = (double *)upload(o, B, sizeof(double) * R * R);
    double *dA = (double *)upload(o, A, sizeof(double) * J * R);
    double *dC = (double *)upload(o, C, sizeof(double) * K * R);
    double *dQ = (double *)upload(o, Q, nQ), *dP = (double *)upload(o, P, nQ), *dT = (double *)upload(o, T, nT);
    int *dS = (int *)upload(o, status, nS);
    char *dY = (char *)upload(o, Y, nY);
    double *dout = out ? (double *)upload(o, out, sizeof(double) * 3) : nullptr;
    Ops::Parafac2Step s;
    s.I = I, s.J = J, s.K = K, s.R = R;
    s.X = dX, s.vdt = vdt, s.s1 = s1, s.s2 = s2;
    s.B = dB, s.A = dA, s.C = dC;
    s.Q = dQ + g, s.P = dP + g, s.T = dT + g, s.status = dS + g;
    s.min_ratio = min_ratio;
    s.Y = dY + ye * g, s.dt = dt, s.out = dout;
    std::vector<std::string> log;
    o.route_log = &log;
    o.parafac2_step(s, nullptr);
    o.route_log = nullptr;
    o.d2h(Q, dQ, nQ);
    o.d2h(P, dP, nQ);
    o.d2h(T, dT, nT);
    o.d2h(status, dS, nS);
    o.d2h(Y, dY, nY);
    if (out) o.d2h(out, dout, sizeof(double) * 3);
    for (void *p : {dX, (void *)dB, (void *)dA, (void *)dC, (void *)dQ, (void *)dP, (void *)dT, (void *)dS, (void *)dY})
      o.free(p);
    if (dout) o.free(dout);
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

// Ops::parafac2_init on P: `guard` doubles, then I R K, then `guard` doubles, prefilled by the caller and copied
// back whole. Returns 0, or -1 with parafac2_shim_error().
int parafac2_shim_init(double *P, int64_t I, int R, int64_t K, int64_t guard) {
  try {
    Ops &o = ops();
    const size_t nP = sizeof(double) * (2 * (size_t)guard + (size_t)I * R * K);
    double *dP = (double *)upload(o, P, nP);
    o.parafac2_init(dP + guard, I, R, K);
    o.d2h(P, dP, nP);
    o.free(dP);
    return 0;
  } catch (const std::exception &e) {
    g_err = e.what();
  } catch (...) {
    g_err = "unknown exception";
  }
  return -1;
}

void parafac2_shim_close() {
  try {
    delete g_ops;
  } catch (...) {
  }
  g_ops = nullptr;
}
}
