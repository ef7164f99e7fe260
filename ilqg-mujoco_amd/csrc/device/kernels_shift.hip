// Receding-horizon shift (ilqg_solver_shift_horizon): the in-place move of the
// per-point arrays, and the store of the tail.  The tail itself is the passive
// rollout kernels' (kernels_rollout.hip, a rollout of horizon n from
// ShiftArgs.carry) and its records are the two-kernel FD sweep's: this unit has
// no physics.
// Nominal refresh (ilqg_solver_refresh_nominal): the cost of the stored nominal
// under the rows in force, summed as the rollout sums it (k_nominal_cost).
// coop_common.h is included for step_cost alone -- the one definition the
// rollout charges with; none of its physics is instantiated here.
#include "coop_common.h"

namespace ilqg {
namespace {

// points a thread has in flight: loaded into registers, then stored
constexpr int SHIFT_U = 8;
constexpr int SHIFT_THREADS = 64;

// One workgroup (one wavefront) per (seed, array, 64-column slice).  A thread
// owns one column c of its array -- one double of every point's slot -- and
// walks the points from N down to n: a[p][c] = a[p - n][c].  It is the only
// thread that reads or writes column c, and in program order every store goes
// to a point above every point still to be read (a block of SHIFT_U points
// stores to [p - U + 1, p] after loading all of [p - U + 1 - n, p - n]; later
// blocks read points <= p - U - n), so the move is correct in place for every
// n in 1 .. N without a barrier, n > P/2 and n = N included.  Consecutive
// threads take consecutive columns: a wavefront reads and writes 512
// contiguous bytes of one point's slot (the FD records are padded to whole
// 128-byte lines).
// Behind the move, the same thread: zero gains below n (the tail has no
// control law), dinit = new point N, carry = new point n (the state the tail's
// rollout starts from) -- values of its own column that it has just written.
__global__ __launch_bounds__(SHIFT_THREADS) void k_shift_horizon(ShiftArgs a) {
  const int arr = blockIdx.y, s = blockIdx.z;
  const int w = a.w[arr];
  const int c = blockIdx.x * SHIFT_THREADS + threadIdx.x;
  if (c >= w) return;
  const int n = a.n, N = a.P - 1;
  const size_t W = (size_t)w;
  double* col = a.arr[arr] + (size_t)s * a.P * W + c;
  int p = N;
  for (; p - (SHIFT_U - 1) >= n; p -= SHIFT_U) {
    double v[SHIFT_U];
#pragma unroll
    for (int q = 0; q < SHIFT_U; q++) v[q] = col[(size_t)(p - q - n) * W];
#pragma unroll
    for (int q = 0; q < SHIFT_U; q++) col[(size_t)(p - q) * W] = v[q];
  }
  for (; p >= n; p--) col[(size_t)p * W] = col[(size_t)(p - n) * W];
  if (arr == ShiftArgs::ARR_K || arr == ShiftArgs::ARR_k)
    for (p = 0; p < n; p++) col[(size_t)p * W] = 0.0;
  if (arr < 5) {
    a.dinit[arr][(size_t)s * W + c] = col[(size_t)N * W];
    a.carry[arr][(size_t)s * W + c] = col[(size_t)n * W];
  }
}

// One workgroup per (seed, tail array, 64-column slice); a thread owns one column
// and copies points n-1 .. 0 of the compact tail (n + 1 points per seed) into
// the resident array (P points per seed).  Source and destination are different
// buffers: no ordering to keep.
__global__ __launch_bounds__(SHIFT_THREADS) void k_shift_store(ShiftArgs a) {
  const int t = blockIdx.y, s = blockIdx.z;
  const int arr = t < 5 ? t : ShiftArgs::ARR_DERIV;
  const int w = a.w[arr];
  const int c = blockIdx.x * SHIFT_THREADS + threadIdx.x;
  if (c >= w) return;
  const int n = a.n;
  const size_t W = (size_t)w;
  double* dst = a.arr[arr] + (size_t)s * a.P * W + c;
  const double* src = a.tail[t] + (size_t)s * (n + 1) * W + c;
  for (int p = 0; p < n; p++) dst[(size_t)p * W] = src[(size_t)p * W];
}

// points a workgroup of k_nominal_cost charges per pass: the LDS it holds, whatever P is
constexpr int NOMC_TILE = 256;

// One workgroup per seed.  a.compute: thread i of a pass takes point hi - i and
// forms its subtotal exactly as the rollout does, step_cost from 0 in (q, v, u)
// order under row (s, n); the subtotals go to LDS and thread 0 adds them to c
// in the rollout's order n = N, N-1, .., 0 (rollout_body.h: c = 0; c +=
// step_cost(point n)), carrying c from one pass of NOMC_TILE points to the next:
// the same additions on the same operands, so the same bits.  !a.compute
// (behind a rollout that charged the nominal into cost_sel itself): c is that
// cost, and dinit takes point N as the selection's setDInit does.
// Thread 0 then publishes: the selected cost, and in the regularisation mode
// cost_nom, valid = 1 and -- a.resume -- status 1 -> 0.
__global__ __launch_bounds__(NOMC_TILE) void k_nominal_cost(NomCostArgs a) {
  __shared__ double sub[NOMC_TILE];
  const int s = blockIdx.x, t = threadIdx.x, N = a.P - 1;
  const int nq = a.nq, nv = a.nv, nu = a.nu;
  double c = 0;
  if (a.compute) {
    const struct { int nq, nv, nu; } m{nq, nv, nu};
    for (int hi = N; hi >= 0; hi -= NOMC_TILE) {
      const int n = hi - t;
      if (n >= 0) {
        const size_t pt = (size_t)s * a.P + n;
        sub[t] = step_cost(m, cost_at(a.cost, s, a.sstride, n, a.cstride), a.nom.qpos + pt * nq, a.nom.qvel + pt * nv,
                           a.nom.ctrl + pt * nu);
      }
      __syncthreads();
      if (t == 0) {
        const int cnt = hi + 1 < NOMC_TILE ? hi + 1 : NOMC_TILE;
        for (int i = 0; i < cnt; i++) c += sub[i];
      }
      __syncthreads();
    }
  } else {
    if (t == 0) c = a.cost_sel[s];
    // setDInit(dArray[N]), inc/ilqr.h:183
    const size_t sp = (size_t)s * a.P + N;
    if (t == 0) a.dinit.time[s] = a.nom.time[sp];
    for (int i = t; i < nq; i += NOMC_TILE) a.dinit.qpos[(size_t)s * nq + i] = a.nom.qpos[sp * nq + i];
    for (int i = t; i < nv; i += NOMC_TILE) {
      a.dinit.qvel[(size_t)s * nv + i] = a.nom.qvel[sp * nv + i];
      a.dinit.warm[(size_t)s * nv + i] = a.nom.warm[sp * nv + i];
    }
    for (int i = t; i < nu; i += NOMC_TILE) a.dinit.ctrl[(size_t)s * nu + i] = a.nom.ctrl[sp * nu + i];
  }
  if (t != 0) return;
  if (a.compute) a.cost_sel[s] = c;
  if (a.rg.cost_nom) {
    a.rg.cost_nom[s] = c;
    a.rg.valid[s] = 1;
    if (a.resume && a.rg.status[s] == 1) a.rg.status[s] = 0;
  }
}

}  // namespace

hipError_t launch_nominal_cost(const NomCostArgs& a, hipStream_t st) {
  if (a.S < 1 || a.P < 1 || a.nq < 1 || a.nv < 1 || a.nu < 0 || !a.cost_sel || !a.nom.qpos || !a.nom.qvel ||
      !a.nom.ctrl)
    return hipErrorInvalidValue;
  if (a.compute && !a.cost.wq) return hipErrorInvalidValue;
  if (!a.compute && (!a.nom.time || !a.nom.warm || !a.dinit.time || !a.dinit.qpos || !a.dinit.qvel ||
                     !a.dinit.warm || !a.dinit.ctrl))
    return hipErrorInvalidValue;
  if (a.rg.cost_nom && (!a.rg.valid || !a.rg.status)) return hipErrorInvalidValue;
  if (a.resume && !a.rg.cost_nom) return hipErrorInvalidValue;
  return launch(k_nominal_cost, (unsigned)a.S, (unsigned)NOMC_TILE, 0, st, a);
}

hipError_t launch_shift_store(const ShiftArgs& a, hipStream_t st) {
  if (a.S < 1 || a.P < 2 || a.n < 1 || a.n > a.P - 1) return hipErrorInvalidValue;
  int wmax = a.w[ShiftArgs::ARR_DERIV];
  for (int t = 0; t < ShiftArgs::NTAIL; t++) {
    const int arr = t < 5 ? t : ShiftArgs::ARR_DERIV;
    if (!a.tail[t] || !a.arr[arr] || a.w[arr] < 1) return hipErrorInvalidValue;
    wmax = a.w[arr] > wmax ? a.w[arr] : wmax;
  }
  const dim3 grid((wmax + SHIFT_THREADS - 1) / SHIFT_THREADS, ShiftArgs::NTAIL, a.S);
  hipLaunchKernelGGL(k_shift_store, grid, dim3(SHIFT_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_shift_horizon(const ShiftArgs& a, hipStream_t st) {
  if (a.S < 1 || a.P < 2 || a.n < 1 || a.n > a.P - 1) return hipErrorInvalidValue;
  int wmax = 0;
  for (int i = 0; i < ShiftArgs::NARR; i++) {
    if (!a.arr[i] || a.w[i] < 1) return hipErrorInvalidValue;
    if (i < 5 && (!a.dinit[i] || !a.carry[i])) return hipErrorInvalidValue;
    wmax = a.w[i] > wmax ? a.w[i] : wmax;
  }
  const dim3 grid((wmax + SHIFT_THREADS - 1) / SHIFT_THREADS, ShiftArgs::NARR, a.S);
  hipLaunchKernelGGL(k_shift_horizon, grid, dim3(SHIFT_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace ilqg
