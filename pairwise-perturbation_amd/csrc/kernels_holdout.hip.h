// kernels_holdout.hip.h — hold-out rows of one mode per start of a multi-start session (Ops::cp_hold_rows).
// wave_sum and gram_pairs come from kernels_small.hip.h.
#pragma once
#include "kernels_small.hip.h"

namespace ppals {

// What follows the update of the sample mode in a hold-out session, for all starts in ONE launch: a
// 1024-thread workgroup per start (StartTable by value, as k_gram_ragged). A start whose bit of `holds` is
// clear returns at once: nothing of it is read or written. Otherwise, on the start's R_b columns from col[b]:
//
//   1. wave w takes the columns w, w + 16, ..., its lanes stride the rows of a column (coalesced). keep[b, x]
//      == 0: the row's entry moves from W into scores, and W and grad get 0; else scores gets 0 and grad^2
//      is added to the lane's sum. Every entry of the block is visited by exactly one lane.
//   2. gradsq[b]: the lanes' sums in the order of wave_sum, then the 16 waves' in ascending order by thread 0.
//   3. behind a barrier, the Gram of the zeroed block into Gall + N sq[b] + mode R_b^2, the 16 waves sharing
//      the R_b (R_b + 1) / 2 pairs: a pair's sum is that of k_gram.
//
// No atomics, every sum in a fixed order: the same state gives the same bits. W, grad and scores do not
// overlap (three buffers of the session); they are not declared restrict because step 3 reads what step 1
// wrote through W.
__global__ __launch_bounds__(1024) void k_cp_hold_rows(double *W, int64_t ldw, double *grad, int64_t ldg,
                                                       double *scores, int64_t lds, int64_t rows, StartTable t,
                                                       const uint8_t *__restrict__ keep, unsigned holds, int N,
                                                       int mode, double *Gall, double *gradsq) {
  __shared__ double part[16];
  const int b = blockIdx.x;
  if (!((holds >> b) & 1u)) return;  // (block-uniform)
  const int R = t.col[b + 1] - t.col[b];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double *w = W + (int64_t)t.col[b] * ldw;
  double *g = grad + (int64_t)t.col[b] * ldg;
  double *sc = scores + (int64_t)t.col[b] * lds;
  const uint8_t *kp = keep + (int64_t)b * rows;
  double acc = 0;
  for (int r = wid; r < R; r += nw)
    for (int64_t x = lane; x < rows; x += 64) {
      if (kp[x]) {
        sc[x + lds * r] = 0.0;
        const double gv = g[x + ldg * r];
        acc += gv * gv;
      } else {
        sc[x + lds * r] = w[x + ldw * r];
        w[x + ldw * r] = 0.0;
        g[x + ldg * r] = 0.0;
      }
    }
  acc = wave_sum(acc);
  if (lane == 0) part[wid] = acc;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int k = 0; k < nw; k++) s += part[k];
    gradsq[b] = s;
  }
  gram_pairs(w, rows, ldw, R, Gall + (int64_t)N * t.sq[b] + (int64_t)mode * R * R, wid, nw);
}

}  // namespace ppals
