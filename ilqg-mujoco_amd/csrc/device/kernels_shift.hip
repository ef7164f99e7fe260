// Receding-horizon shift (ilqg_solver_shift_horizon): the in-place move of the
// per-point arrays, and the store of the tail.  The tail itself is the passive
// rollout kernels' (kernels_rollout.hip, a rollout of horizon n from
// ShiftArgs.carry) and its records are the two-kernel FD sweep's: this unit has
// no physics.
#include "kernels.h"

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

}  // namespace

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
