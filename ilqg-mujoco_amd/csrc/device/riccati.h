// initV + Riccati backward pass (inc/ilqr.h:100-107,133-176) for one seed on
// one 64-lane wavefront, every matrix LDS-resident: the body of k_backward
// (riccati.hip) and the backward role of the fused FD sweep (kernels_coop.hip),
// which streams the FD records in as the sweep publishes them.
//
// Same loops, same summation order as oracle/ilqr_ora.c ora_riccati_step, so
// K, k, V, v are bit-identical to the oracle.  Templated on (NV, NU): the
// bundled models' sizes get compile-time loop bounds and index arithmetic;
// <0,0> is the generic instance.  Square matrices use a padded leading
// dimension nx+1 so the strided column walks spread over the LDS banks.
#pragma once
#include <hip/hip_runtime.h>

#include "dphys.h"
#include "handoff.h"
#include "kernels.h"

#ifndef BSTAMP
#define BSTAMP(id) \
  do {             \
  } while (0)
#endif

#include "riccati_reg.h"

namespace ilqg {

constexpr int BW_THREADS = 64;  // one wavefront: its barriers compile to nothing
constexpr int BW_PF = 8;        // prefetch registers per lane: D <= 512


// Eigen-style LDLT with symmetric pivoting (oracle ora_ldlt_factor); lane 0.
// temp: n doubles of LDS scratch (a private array would live in scratch memory)
__device__ inline void ldlt_factor(int n, double* mat, int* transp, double* temp) {
  for (int k = 0; k < n; k++) {
    int big = k;
    double bigv = fabs(mat[k + k * n]);
    int rs = n - k - 1;
    for (int i = k + 1; i < n; i++)
      if (fabs(mat[i + i * n]) > bigv) { bigv = fabs(mat[i + i * n]); big = i; }
    transp[k] = big;
    if (k != big) {
      int s = n - big - 1;
      double t;
      for (int j = 0; j < k; j++) { t = mat[k + j * n]; mat[k + j * n] = mat[big + j * n]; mat[big + j * n] = t; }
      for (int i = 0; i < s; i++) {
        t = mat[(big + 1 + i) + k * n];
        mat[(big + 1 + i) + k * n] = mat[(big + 1 + i) + big * n];
        mat[(big + 1 + i) + big * n] = t;
      }
      t = mat[k + k * n]; mat[k + k * n] = mat[big + big * n]; mat[big + big * n] = t;
      for (int i = k + 1; i < big; i++) { t = mat[i + k * n]; mat[i + k * n] = mat[big + i * n]; mat[big + i * n] = t; }
    }
    if (k > 0) {
      double s = 0;
      for (int j = 0; j < k; j++) temp[j] = mat[j + j * n] * mat[k + j * n];
      for (int j = 0; j < k; j++) s += mat[k + j * n] * temp[j];
      mat[k + k * n] -= s;
      for (int i = k + 1; i < n; i++) {
        double si = 0;
        for (int j = 0; j < k; j++) si += mat[i + j * n] * temp[j];
        mat[i + k * n] -= si;
      }
    }
    if (k == 0 && !(fabs(mat[0]) > 0)) {
      for (int j = 0; j < n; j++) transp[j] = j;
      return;
    }
    if (rs > 0 && fabs(mat[k + k * n]) > 0)
      for (int i = k + 1; i < n; i++) mat[i + k * n] /= mat[k + k * n];
  }
}
// The same factorization by one wavefront (lane = the calling thread's lane,
// every lane of the wave calls it; n <= 32): each matrix entry receives
// exactly ldlt_factor's operations in ldlt_factor's order -- the pivot scan,
// the four swap groups (disjoint entries: one lane each), temp, the dot
// products of row k and of every row below it (one lane per row, ascending j)
// and the column scaling -- so the factor is bit-identical; the phases of
// column k are separated by wavefront-scope barriers.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ inline void ldlt_factor_wave(int n, double* mat, int* transp, double* temp, int lane) {
  for (int k = 0; k < n; k++) {
    // pivot: the first row of largest |diagonal| among k..n-1 (strict >, as the oracle)
    const double dg = (lane >= k && lane < n) ? fabs(mat[lane + lane * n]) : 0.0;
    int big = k;
    double bigv = __shfl(dg, k);
    for (int i = k + 1; i < n; i++) {
      const double a = __shfl(dg, i);
      if (a > bigv) {
        bigv = a;
        big = i;
      }
    }
    if (lane == 0) transp[k] = big;
    if (k != big) {
      const int s = n - big - 1;
      double t;
      if (lane < k) {  // row k <-> row big, columns j < k
        const int j = lane;
        t = mat[k + j * n]; mat[k + j * n] = mat[big + j * n]; mat[big + j * n] = t;
      }
      if (lane < s) {  // rows below big: column k <-> column big
        const int i = lane;
        t = mat[(big + 1 + i) + k * n];
        mat[(big + 1 + i) + k * n] = mat[(big + 1 + i) + big * n];
        mat[(big + 1 + i) + big * n] = t;
      }
      if (lane == 32) {
        t = mat[k + k * n]; mat[k + k * n] = mat[big + big * n]; mat[big + big * n] = t;
      }
      if (lane > 32 + k && lane < 32 + big) {  // between: column k <-> row big
        const int i = lane - 32;
        t = mat[i + k * n]; mat[i + k * n] = mat[big + i * n]; mat[big + i * n] = t;
      }
    }
    wave_sync();
    if (k > 0) {
      if (lane < k) temp[lane] = mat[lane + lane * n] * mat[k + lane * n];
      wave_sync();
      // lane i >= k: row i's dot with temp (row k: the diagonal update)
      if (lane >= k && lane < n) {
        double si = 0;
        for (int j = 0; j < k; j++) si += mat[lane + j * n] * temp[j];
        mat[lane + k * n] -= si;
      }
      wave_sync();
    }
    if (k == 0 && !(fabs(mat[0]) > 0)) {
      for (int j = lane; j < n; j += 64) transp[j] = j;
      wave_sync();
      return;
    }
    const double d = mat[k + k * n];
    if (n - k - 1 > 0 && fabs(d) > 0 && lane > k && lane < n) mat[lane + k * n] /= d;
    wave_sync();
  }
}

__device__ inline void ldlt_solve(int n, const double* Lm, const int* transp, double* x) {
  const double tol = 2.2250738585072014e-308;
  for (int k = 0; k < n; k++) { double t = x[k]; x[k] = x[transp[k]]; x[transp[k]] = t; }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++) x[i] -= Lm[i + j * n] * x[j];
  for (int i = 0; i < n; i++) {
    if (fabs(Lm[i + i * n]) > tol) x[i] /= Lm[i + i * n];
    else x[i] = 0;
  }
  for (int i = n - 1; i >= 0; i--)
    for (int j = i + 1; j < n; j++) x[i] -= Lm[j + i * n] * x[j];
  for (int k = n - 1; k >= 0; k--) { double t = x[k]; x[k] = x[transp[k]]; x[transp[k]] = t; }
}

// ldlt_solve with the vector in registers (n <= 32, every index a compile-time
// constant): the pivot swaps before and after the substitutions are one
// gather and one scatter through perm (ldlt_perm), and every entry receives
// ldlt_solve's operations in ldlt_solve's order.  Lm reads are uniform LDS
// loads independent of x, so they issue ahead of the dependent chain.
// Each calling lane solves its own vector x (active lanes only).
// perm[i] = the source position of entry i after ldlt_solve's forward swaps:
// lane i applies the transpositions to its index, last one first
__device__ inline void ldlt_perm(int n, const int* transp, int* perm, int lane) {
  if (lane < n) {
    int p = lane;
    for (int k = n - 1; k >= 0; k--) {
      const int t = transp[k];
      p = p == k ? t : (p == t ? k : p);
    }
    perm[lane] = p;
  }
}
__device__ inline void ldlt_solve_reg(int n, const double* Lm, const int* perm, double* x, bool active) {
  constexpr int NM = 32;
  const double tol = 2.2250738585072014e-308;
  double r[NM];
  rreg::sf<0, NM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    r[i] = (active && i < n) ? x[perm[i]] : 0.0;
  });
  rreg::sf<0, NM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    if (i < n)
      rreg::sf<0, i>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        r[i] -= Lm[i + j * n] * r[j];
      });
  });
  rreg::sf<0, NM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    if (i < n) {
      const double d = Lm[i + i * n];
      r[i] = fabs(d) > tol ? r[i] / d : 0.0;
    }
  });
  rreg::sf<0, NM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = NM - 1 - decltype(ii)::value;
    if (i < n)
      rreg::sf<i + 1, NM>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        if (j < n) r[i] -= Lm[j + i * n] * r[j];
      });
  });
  rreg::sf<0, NM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    if (active && i < n) x[perm[i]] = r[i];
  });
}

// ldlt_factor_wave and ldlt_solve_reg for a compile-time size N (the MFMA
// engine's humanoid instance, nu = 21): every loop unrolled, no size guards.
// The pivot scan is a wave max-reduction instead of the serial shuffle chain:
// |diagonal| >= 0, so its IEEE bits order like the values; rows whose
// |diagonal| is NaN take key 0 (the strict > of the scan never picks them), a
// NaN at row k keeps k (the scan never moves), and the first row attaining the
// maximum is the scan's choice (a tie at key 0 includes row k itself).
// max(x, x rotated right by S lanes within its 16-lane row) (DPP row_ror)
template <int S>
__device__ __forceinline__ unsigned long long umax_ror(unsigned long long x) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)x, 0x120 + S, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), 0x120 + S, 0xf, 0xf, false);
  const unsigned long long y = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  return y > x ? y : x;
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long x, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
template <int N>
__device__ inline void ldlt_factor_wave_t(double* mat, int* transp, double* temp, int lane) {
  static_assert(N >= 1 && N <= 32, "one wavefront, n <= 32");
  bool stop = false;
  rreg::sf<0, N>([&](auto kk) __attribute__((always_inline)) {
    constexpr int k = decltype(kk)::value;
    if (stop) return;
    const bool in = lane >= k && lane < N;
    const int li = lane < N ? lane : N - 1;
    const double dg = fabs(mat[li + li * N]);
    unsigned long long key = (in && dg == dg) ? (unsigned long long)__double_as_longlong(dg) : 0ull;
    // max over each 16-lane row by DPP row rotations, then rows 0 and 1 (n <= 32)
    key = umax_ror<8>(key);
    key = umax_ror<4>(key);
    key = umax_ror<2>(key);
    key = umax_ror<1>(key);
    const unsigned long long m0 = readlane_u64(key, 0), m1 = readlane_u64(key, 16);
    const unsigned long long kmax = m1 > m0 ? m1 : m0;
    const double dk = fabs(mat[k + k * N]);
    int big = k;
    if (dk == dk) {
      const unsigned long long hit = __ballot(in && dg == dg && (unsigned long long)__double_as_longlong(dg) == kmax);
      // kmax == 0: every candidate is 0 or NaN, row k (0) the first of them
      if (kmax != 0ull) big = (int)__builtin_ctzll(hit);
    }
    if (lane == 0) transp[k] = big;
    if (k != big) {
      const int s = N - big - 1;
      double t;
      if (lane < k) {  // row k <-> row big, columns j < k
        const int j = lane;
        t = mat[k + j * N]; mat[k + j * N] = mat[big + j * N]; mat[big + j * N] = t;
      }
      if (lane < s) {  // rows below big: column k <-> column big
        const int i = lane;
        t = mat[(big + 1 + i) + k * N];
        mat[(big + 1 + i) + k * N] = mat[(big + 1 + i) + big * N];
        mat[(big + 1 + i) + big * N] = t;
      }
      if (lane == 32) {
        t = mat[k + k * N]; mat[k + k * N] = mat[big + big * N]; mat[big + big * N] = t;
      }
      if (lane > 32 + k && lane < 32 + big) {  // between: column k <-> row big
        const int i = lane - 32;
        t = mat[i + k * N]; mat[i + k * N] = mat[big + i * N]; mat[big + i * N] = t;
      }
    }
    wave_sync();
    if constexpr (k > 0) {
      if (lane < k) temp[lane] = mat[lane + lane * N] * mat[k + lane * N];
      wave_sync();
      // lane i >= k: row i's dot with temp (row k: the diagonal update), ascending j
      double a[k], b[k];
      rreg::sf<0, k>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        a[j] = mat[li + j * N];
        b[j] = temp[j];
      });
      double si = 0;
      rreg::sf<0, k>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        si += a[j] * b[j];
      });
      if (in) mat[lane + k * N] -= si;
      wave_sync();
    }
    if constexpr (k == 0) {
      if (!(fabs(mat[0]) > 0)) {
        for (int j = lane; j < N; j += 64) transp[j] = j;
        wave_sync();
        stop = true;
        return;
      }
    }
    if constexpr (N - k - 1 > 0) {
      const double d = mat[k + k * N];
      if (fabs(d) > 0 && lane > k && lane < N) mat[lane + k * N] /= d;
    }
    wave_sync();
  });
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
  return __longlong_as_double((long long)readlane_u64((unsigned long long)__double_as_longlong(x), l));
}
// ldlt_factor_wave_t's factor with the matrix in registers, one row per lane.
// ldlt_factor's pivot scan reads the diagonal entries of rows k..n-1, which no
// earlier column has updated (entry (k, k) is updated at step k), so the pivot
// sequence is a function of the input's diagonal alone: it is replayed first
// (lane q holds the key of the row at position q; ldlt_factor_wave_t's scan and
// row swaps on the keys), which also yields the rows' final order -- perm,
// what ldlt_perm derives from transp.  Lane i then holds row perm[i] of the
// (lower-triangle) symmetric input in that order and forms column k with
// ldlt_factor's operations in ldlt_factor's order: temp[j] = D[j] L(k, j)
// (lane k's products, read across the wave with v_readlane), the row's dot
// product with temp ascending from +0, its subtraction from the input entry,
// the division by the updated diagonal.  The factor is the same bit for bit
// (tests/test_gpu_parity.py::test_ldlt_reg_matches_lds; with tied, zero,
// denormal and NaN keys tests/test_riccati_cases.py::test_mfma_engine); a NaN
// or an all-zero diagonal (ldlt_factor's early exit) takes ldlt_factor_wave_t
// + ldlt_perm.
// Writes the lower triangle and diagonal of mat, and perm.  transp is NOT
// written on the register path (only the NaN / all-zero fallback writes it):
// it keeps whatever an earlier step left, and perm alone carries the pivot
// order to the solves.
// (replay: the replay even without equal keys, for the test)
template <int N>
__device__ inline void ldlt_factor_reg_t(double* mat, int* transp, int* perm, double* temp, int lane,
                                         bool replay = false) {
  static_assert(N >= 1 && N <= 32, "one wavefront, n <= 32");
  const int li = lane < N ? lane : N - 1;
  const double dg = fabs(mat[li + li * N]);
  const unsigned long long key0 = lane < N ? (unsigned long long)__double_as_longlong(dg) : 0ull;
  if (__ballot(lane < N && dg != dg) != 0ull || __ballot(lane < N && dg > 0) == 0ull) {
    ldlt_factor_wave_t<N>(mat, transp, temp, lane);
    ldlt_perm(N, transp, perm, lane);
    return;
  }
  // the pivot sequence.  Distinct keys: the scan picks the largest remaining
  // key whatever the rows' positions, so the order is the rows by |diagonal|
  // descending -- each lane counts the keys above its own.  Equal keys (the
  // first in the current order wins, and the swaps reorder the rest): the scan
  // and its swaps replayed on the keys, lane q holding position q's row and key.
  int rank = 0;
  bool tie = false;
  rreg::sf<0, N>([&](auto jj) __attribute__((always_inline)) {
    constexpr int j = decltype(jj)::value;
    const double dj = fabs(mat[j + j * N]);
    rank += dj > dg ? 1 : 0;
    tie = tie || (lane < N && lane != j && dj == dg);
  });
  int pos;
  if (__ballot(tie) == 0ull && !replay) {
    if (lane < N) perm[rank] = lane;
    wave_sync();
    pos = lane < N ? perm[lane] : 0;
  } else {
    pos = lane < N ? lane : 0;
    unsigned long long ky = key0;
    rreg::sf<0, N>([&](auto kk) __attribute__((always_inline)) {
      constexpr int k = decltype(kk)::value;
      const bool in = lane >= k && lane < N;
      unsigned long long key = in ? ky : 0ull;
      key = umax_ror<8>(key);
      key = umax_ror<4>(key);
      key = umax_ror<2>(key);
      key = umax_ror<1>(key);
      const unsigned long long m0 = readlane_u64(key, 0), m1 = readlane_u64(key, 16);
      const unsigned long long kmax = m1 > m0 ? m1 : m0;
      const unsigned long long hit = __ballot(in && ky == kmax);
      const int big = kmax != 0ull ? (int)__builtin_ctzll(hit) : k;
      if (big != k) {
        const unsigned long long kb = readlane_u64(ky, big), kk0 = readlane_u64(ky, k);
        const int pb = __builtin_amdgcn_readlane(pos, big), pk = __builtin_amdgcn_readlane(pos, k);
        if (lane == k) {
          ky = kb;
          pos = pb;
        } else if (lane == big) {
          ky = kk0;
          pos = pk;
        }
      }
    });
    if (lane < N) perm[lane] = pos;
  }
  // row pos of the symmetric input, columns in the final order (all reads issue
  // before the first write below)
  double a[N];
  rreg::sf<0, N>([&](auto cc) __attribute__((always_inline)) {
    constexpr int c = decltype(cc)::value;
    const int pc = __builtin_amdgcn_readlane(pos, c);
    const int hi = pos > pc ? pos : pc, lo = pos > pc ? pc : pos;
    a[c] = mat[hi + lo * N];
  });
  // the column loop is one basic block (no stores, no branches), so the
  // scheduler can start column k's dot products beside column k-1's division
  double l[N], dl[N];  // L(i, j); D[j] L(i, j)
  double dd = 0;       // lane i: D[i]
  rreg::sf<0, N>([&](auto kk) __attribute__((always_inline)) {
    constexpr int k = decltype(kk)::value;
    double v = a[k];
    if constexpr (k > 0) {
      double si = 0;
      rreg::sf<0, k>([&](auto jj) __attribute__((always_inline)) {
        constexpr int j = decltype(jj)::value;
        si += l[j] * readlane_f64(dl[j], k);
      });
      v -= si;
    }
    const double d = readlane_f64(v, k);
    dd = lane == k ? d : dd;
    if constexpr (N - k - 1 > 0) {
      const double lk = fabs(d) > 0 ? v / d : v;
      l[k] = lk;
      dl[k] = d * lk;
    }
  });
  // column j of lane i: L(i, j) below the diagonal; the lanes above it write
  // their (unused) values into the upper triangle, which nothing reads; the
  // diagonal last
  if (lane < N) {
    rreg::sf<0, N - 1>([&](auto jj) __attribute__((always_inline)) {
      constexpr int j = decltype(jj)::value;
      mat[lane + j * N] = l[j];
    });
    mat[lane + lane * N] = dd;
  }
}
// a zero the compiler cannot see through, produced after v: L reads addressed
// with it cannot be hoisted above v's computation (left free, the scheduler
// issues all N^2 reads of an unrolled solve at once and the kernel spills)
__device__ __forceinline__ int zero_after(double v) {
  int z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z) : "v"(v));
  return z;
}
template <int N>
__device__ inline void ldlt_solve_reg_t(const double* Lm, const int* perm, const double* src, double* x, bool dbl,
                                        bool active) {
  const double tol = 2.2250738585072014e-308;
  double r[N];
  // the right-hand side src (2 src when dbl: the caller's doubling, exact),
  // solved into x
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    const double b = active ? src[perm[i]] : 0.0;
    r[i] = dbl ? 2 * b : b;
  });
  // forward substitution column by column: r[i] -= L(i, j) r[j] for i > j --
  // each r[i] still receives its subtractions in ascending j, ldlt_solve's
  // order.  Column j's L reads wait for r[j - 1] (final one column earlier):
  // they overlap the previous column's updates, no further ahead.
  rreg::sf<0, N>([&](auto jj) __attribute__((always_inline)) {
    constexpr int j = decltype(jj)::value;
    const double* Lc = Lm + (j > 0 ? zero_after(r[j > 0 ? j - 1 : 0]) : 0);
    rreg::sf<j + 1, N>([&](auto ii) __attribute__((always_inline)) {
      constexpr int i = decltype(ii)::value;
      r[i] -= Lc[i + j * N] * r[j];
    });
  });
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    const double d = Lm[i + i * N];
    r[i] = fabs(d) > tol ? r[i] / d : 0.0;
  });
  // backward rows, i descending: row i's reads wait for r[i + 2]
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = N - 1 - decltype(ii)::value;
    const double* Lc = Lm + (i + 2 < N ? zero_after(r[i + 2 < N ? i + 2 : 0]) : 0);
    rreg::sf<i + 1, N>([&](auto jj) __attribute__((always_inline)) {
      constexpr int j = decltype(jj)::value;
      r[i] -= Lc[j + i * N] * r[j];
    });
  });
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    if (active) x[perm[i]] = r[i];
  });
}

// x, copied once dep is computed (the copy cannot move above dep)
__device__ __forceinline__ double copy_after(double x, double dep) {
  double y;
  asm volatile("v_mov_b64 %0, %1" : "=v"(y) : "v"(x), "v"(dep));
  return y;
}
// ldlt_solve_reg_t with the factor read across the wave instead of from LDS:
// lane i holds row i of the factor (L(i, j), j < i, and D(i)) in registers,
// loaded once, and every use of L(i, j) is a v_readlane of lane i's register j
// into scalar registers -- no LDS load, so no LDS latency, on the
// substitutions' dependent chain.  The same operations in the same order.
template <int N>
__device__ inline void ldlt_solve_bcast_t(const double* Lm, const int* perm, const double* src, double* x, bool dbl,
                                          bool active, int lane) {
  const double tol = 2.2250738585072014e-308;
  const int li = lane < N ? lane : 0;
  double Lr[N];  // row li of the factor (its upper part unused)
  rreg::sf<0, N>([&](auto jj) __attribute__((always_inline)) {
    constexpr int j = decltype(jj)::value;
    Lr[j] = Lm[li + j * N];
  });
  double r[N];
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    const double b = active ? src[perm[i]] : 0.0;
    r[i] = dbl ? 2 * b : b;
  });
  // (column j's reads are issued once r[j - 1] is final, row i's once r[i + 2]
  // is: left free, the scheduler hoists every read into scalar registers and
  // spills them -- as zero_after does for ldlt_solve_reg_t's LDS reads)
  rreg::sf<0, N>([&](auto jj) __attribute__((always_inline)) {
    constexpr int j = decltype(jj)::value;
    const double Lc = j > 0 ? copy_after(Lr[j], r[j > 0 ? j - 1 : 0]) : Lr[j];
    rreg::sf<j + 1, N>([&](auto ii) __attribute__((always_inline)) {
      constexpr int i = decltype(ii)::value;
      r[i] -= readlane_f64(Lc, i) * r[j];
    });
  });
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    const double d = readlane_f64(Lr[i], i);
    r[i] = fabs(d) > tol ? r[i] / d : 0.0;
  });
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = N - 1 - decltype(ii)::value;
    const double Lc = i + 2 < N ? copy_after(Lr[i], r[i + 2 < N ? i + 2 : 0]) : Lr[i];
    rreg::sf<i + 1, N>([&](auto jj) __attribute__((always_inline)) {
      constexpr int j = decltype(jj)::value;
      r[i] -= readlane_f64(Lc, j) * r[j];
    });
  });
  rreg::sf<0, N>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = decltype(ii)::value;
    if (active) x[perm[i]] = r[i];
  });
}

// Three independent fixed-order dot products per lane (ILP 3): each output
// keeps the oracle's summation order, the three chains overlap in the pipe.
#define ILP3_BEGIN(n)                                    \
  for (int e0 = tid; e0 < (n); e0 += 3 * BW_THREADS) {   \
    const int e1 = e0 + BW_THREADS, e2 = e0 + 2 * BW_THREADS; \
    const bool h1 = e1 < (n), h2 = e2 < (n);             \
    const int f1 = h1 ? e1 : e0, f2 = h2 ? e2 : e0;

// ---- the boxed step (BOX instances of backward_seed; the reference has no
// counterpart).  Trip bounds of its two loops, both compile-time: a step that
// exhausts either takes the fallback, so no input can make the kernel wait.
constexpr int BOX_MAXIT = 32;   // projected-Newton iterations
constexpr int BOX_MAXLS = 24;   // Armijo halvings (0.6^24 ~ 5e-6 of the Newton step)
constexpr double BOX_ARMIJO = 0.1, BOX_SHRINK = 0.6;
// extra LDS of a BOX instance, in doubles: Mm's copy and seven nu-vectors
__host__ __device__ constexpr size_t box_lds_doubles(size_t nu) { return nu * nu + 7 * nu; }
// a wave-uniform flag as a scalar: every lane computed the same value from LDS
__device__ __forceinline__ int box_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double box_clip(double c, double lo, double hi) { return c < lo ? lo : (c > hi ? hi : c); }
// LDS of one boxed step.  Mo: Mm as stage 3 built it (Mm itself is factored in
// place); bl, bh: the bounds on k; x: the iterate; gr: col - Mo x; xt: the
// Newton target; xc, gc: the line search's candidate and its gradient
struct BoxLds {
  double *Mo, *bl, *bh, *x, *gr, *xt, *xc, *gc;
};
// out = col - Mo in: lane a's row, ascending b
__device__ inline void box_grad(int nu, const double* Mo, const double* col, const double* in, double* out, int tid) {
  if (tid < nu) {
    double sm = 0;
    for (int b = 0; b < nu; b++) sm += Mo[tid + b * nu] * in[b];
    out[tid] = col[tid] - sm;
  }
}
// min 1/2 k'(-Mo)k + col'k over bl <= k <= bh by projected Newton (Tassa,
// Mansard & Todorov 2014) from the clamped unconstrained k (kl), one wavefront.
// The clamped set is the controls at a bound whose gradient points outward; the
// Newton target solves the free block -- Mm rebuilt from Mo with every clamped
// row and column replaced by a -1 diagonal entry, the bounds' contribution on
// the right-hand side -- and the step is backtracked with projection until
// Armijo's condition holds.  The iteration ends when a full, unprojected step
// leaves the clamped set unchanged (the iterate is then that set's stationary
// point exactly, not to a gradient tolerance), or every control is clamped.
// Every decision is computed by all lanes from the same LDS values in the same
// order and passed through box_uni: the branches around the barriers are
// wave-uniform.  Returns the clamped set in *mask and the iteration count, or
// -1 for the fallback (a free-block pivot >= 0 or NaN, no acceptable step, or
// BOX_MAXIT reached).  On a regular return with a free control, Mm / trn hold
// the factor of the final set's matrix.
__device__ inline int box_solve(int nu, const BoxLds& L, double* Mm, const double* col, const double* kl, int* trn,
                                double* temp, int tid, unsigned* mask_out) {
  const unsigned full = nu >= 32 ? ~0u : ((1u << nu) - 1u);
  if (tid < nu) L.x[tid] = box_clip(kl[tid], L.bl[tid], L.bh[tid]);
  wave_sync();
  unsigned prev = 0;
  int lastfull = 0, state = 0, iters = 0;  // state: 0 iterating, 1 done, -1 fallback
  unsigned mask = 0;
#pragma unroll 1
  for (int it = 0; it < BOX_MAXIT; it++) {
    if (box_uni(state != 0)) break;
    box_grad(nu, L.Mo, col, L.x, L.gr, tid);
    wave_sync();
    mask = 0;
    for (int a = 0; a < nu; a++) {
      const double xa = L.x[a], ga = L.gr[a];
      if ((xa == L.bl[a] && ga > 0) || (xa == L.bh[a] && ga < 0)) mask |= 1u << a;
    }
    mask = (unsigned)box_uni((int)mask);
    if (box_uni(mask == full || (it > 0 && lastfull && mask == prev))) {
      state = 1;
      break;
    }
    // the free block's matrix and right-hand side
    for (int e = tid; e < nu * nu; e += BW_THREADS) {
      const int a = e % nu, b = e / nu;
      const bool cl = ((mask >> a) | (mask >> b)) & 1u;
      Mm[e] = cl ? (a == b ? -1.0 : 0.0) : L.Mo[e];
    }
    if (tid < nu) {
      double sm = col[tid];
      if ((mask >> tid) & 1u) {
        sm = -L.x[tid];
      } else {
        for (int b = 0; b < nu; b++)
          if ((mask >> b) & 1u) sm -= L.Mo[tid + b * nu] * L.x[b];
      }
      L.xt[tid] = sm;
    }
    wave_sync();
    ldlt_factor_wave(nu, Mm, trn, temp, tid);
    // -Mm_ff must be positive definite: every pivot of the factor negative
    int ok = 1;
    for (int a = 0; a < nu; a++) ok &= Mm[a + a * nu] < 0 ? 1 : 0;
    if (box_uni(!ok)) {
      state = -1;
      break;
    }
    if (tid == 0) ldlt_solve(nu, Mm, trn, L.xt);
    wave_sync();
    if (tid < nu && ((mask >> tid) & 1u)) L.xt[tid] = L.x[tid];
    wave_sync();
    // f(x) = 1/2 x'(-Mo)x + col'x = 1/2 sum x_a (gr_a + col_a)
    double f0 = 0;
    for (int a = 0; a < nu; a++) f0 += L.x[a] * (L.gr[a] + col[a]);
    f0 *= 0.5;
    double step = 1.0;
    int acc = 0;
#pragma unroll 1
    for (int ls = 0; ls < BOX_MAXLS; ls++) {
      if (box_uni(acc)) break;
      // (the full step is the target itself: x + (xt - x) may round to its neighbour)
      if (tid < nu)
        L.xc[tid] = box_clip(step == 1.0 ? L.xt[tid] : L.x[tid] + step * (L.xt[tid] - L.x[tid]), L.bl[tid], L.bh[tid]);
      wave_sync();
      box_grad(nu, L.Mo, col, L.xc, L.gc, tid);
      wave_sync();
      double fc = 0, dec = 0;
      for (int a = 0; a < nu; a++) {
        fc += L.xc[a] * (L.gc[a] + col[a]);
        dec += L.gr[a] * (L.xc[a] - L.x[a]);
      }
      fc *= 0.5;
      acc = box_uni(fc - f0 <= BOX_ARMIJO * dec ? 1 : 0);  // a NaN never accepts
      if (!acc) step *= BOX_SHRINK;
      wave_sync();  // xc, gc are rewritten by the next trial
    }
    if (box_uni(!acc)) {
      state = -1;
      break;
    }
    int fullstep = step == 1.0 ? 1 : 0;
    for (int a = 0; a < nu; a++) fullstep &= L.xc[a] == L.xt[a] ? 1 : 0;
    lastfull = box_uni(fullstep);
    prev = mask;
    wave_sync();
    if (tid < nu) L.x[tid] = L.xc[tid];
    wave_sync();
    iters++;
  }
  *mask_out = mask;
  return box_uni(state) == 1 ? iters : -1;
}

// ---- the standard step (STD instances of backward_seed, ILQG_RECURSION_STANDARD;
// it replaces inc/ilqr.h:157-174, whose outer-product Hessians, resident mu and
// factors of 2 it does not keep).  Deviation coordinates about the nominal
// trajectory (no c term), the exact diagonal Hessians of ilqg_cost from the
// cost row of the step's point, mu in Quu and Qux only (Tassa, Erez & Todorov
// 2012, eq. 10), and the value update in its closed-loop form, which holds for
// any gains:
//   Quu_r = luu + B'(V + mu I)B   Qux_r = B'(V + mu I)A   Qu = r + B'v
//   k = -Quu_r^-1 Qu              K = -Quu_r^-1 Qux_r
//   dV1 += k'Qu                   dV2 += 1/2 k'(luu + B'VB)k
//   V <- lxx + K'luu K + (A+BK)'V(A+BK)
//   v <- q + K'(r + luu k) + (A+BK)'(v + V B k)
// A step whose Quu_r has a pivot <= 0 or NaN (or whose gains come out
// non-finite) takes K = 0, k = 0 and adds nothing to dV (the decision is
// wave-uniform, box_uni).
// extra LDS of an STD instance, in doubles: the unregularised Quu, lxx, luu
__host__ __device__ constexpr size_t std_lds_doubles(size_t nv, size_t nu) { return nu * nu + 2 * nv + nu; }

//
// REG (with STD; RegDev, kernels.h): mu is the seed's own, rg.mu[s], and an
// indefinite step raises it (reg_increase) and restarts the recursion from
// step 1 -- the same V0, v0 (Vg, vg are written only behind the last attempt),
// the record prefetch primed again -- while fewer than rg.max_retry restarts
// were used and rg.status[s] is 0; otherwise the step takes the fallback above.
// The restart is a backward jump taken by the whole wave (box_uni) under a
// counter bounded by the constant REG_MAXRETRY: a pass costs at most
// REG_MAXRETRY + 1 plain passes and waits on nothing.  A jump, not a loop
// around the body, so that the instances without REG compile from the same
// statements as before.

template <int NV_, int NU_, bool BOX = false, bool STD = false, bool REG = false, class MD>
__device__ inline void backward_seed(const MD& m, int nq, int nv_rt, int nu_rt, int P, double dt, double mu,
                                     const double* deriv, int Ds, TrajDev tr, double* Kg, double* kg, double* Vg,
                                     double* vg, int s, int tid, double* sh, const unsigned* done, unsigned target,
                                     unsigned* fault, RicFlags fl, BoxDev bx = BoxDev{}, StdDev sd = StdDev{},
                                     RegDev rg = RegDev{}) {
  static_assert(!(BOX && STD), "the boxed step is the reference recursion's");
  static_assert(!REG || STD, "the restart belongs to the standard step");
#ifndef ILQG_RIC_LDS
  // bundled small models: the register/exchange formulation (riccati_reg.h)
  // (a BOX or STD instance is always the LDS formulation below)
  if constexpr (!BOX && !STD && RicReg<NV_, NU_>::ok) {
    if (nq == NV_) {
      backward_seed_reg<NV_, NU_>(m, P, dt, mu, deriv, Ds, tr, Kg, kg, Vg, vg, s, tid, sh, done, target, fault, fl);
      return;
    }
  }
#endif
  const int nv = NV_ > 0 ? NV_ : nv_rt;
  const int nu = NU_ > 0 ? NU_ : nu_rt;
  const int nx = 2 * nv, D = nv * (2 * nv + nu) + 2 * nv + nu;
  // padded leading dimension of the nx-row matrices (unpadded for large nx,
  // where LDS capacity binds)
  const int LX = nx <= 32 ? nx + 1 : nx;
  // FD record prefetched into LDS (always, when streaming from the FD sweep)
  const bool pref = D <= BW_PF * BW_THREADS;
  // streaming (done != nullptr): record p is read only once its FD teams have
  // all published it (done[s P + p] >= target), with sc1 loads
  // (the flags of records up to ready_upto were seen published by an earlier poll)
  int ready_upto = -1;
  auto ready = [&](int p) {
    if (!done || p <= ready_upto) return;
#ifdef ILQG_STAMPS
    const unsigned long long t0_ = __builtin_amdgcn_s_memtime();
#endif
    ready_upto = bw_wait_window(done + (size_t)s * P, p, P, target, fault);
#ifdef ILQG_STAMPS
    if (s == 0 && tid == 0) {
      g_fused_diag[1] += __builtin_amdgcn_s_memtime() - t0_;
      g_fused_diag[2]++;
    }
    if (s < 8 && tid == 0) g_fused_diag[16 + s] += __builtin_amdgcn_s_memtime() - t0_;
#endif
  };
  auto ld = [&](const double* a) -> double { return done ? ld_sc1(a) : *a; };
  // buffers are reused once dead: V holds V_new (V is read only by stage 1),
  // A holds T4 (A is last read in stage 5)
  double* V = sh;                 // nx x nx, ld LX; V_new from stage 7
  double* Vs = V + nx * LX;
  double* A = Vs + nx * LX;       // T4 from stage 6
  double* ABK = A + nx * LX;
  double* B = ABK + nx * LX;      // nx x nu, ld LX
  double* T6 = B + nu * LX;       // nx x nu, ld LX
  double* T1 = T6 + nu * LX;      // nu x nx, ld nu
  double* T3 = T1 + nu * nx;
  double* Kl = T3 + nu * nx;
  double* Mm = Kl + nu * nx;      // nu x nu
  double* v = Mm + nu * nu;
  double* c = v + nx;
  double* w = c + nx;
  double* y = w + nx;
  double* z = y + nx;
  double* vn = z + nx;
  double* q = vn + nx;
  double* kl = q + nx;
  double* kR = kl + nu;
  double* col = kR + nu;
  double* r = col + nu;
  double* dl = r + nu;  // FD record of the current step (prefetched), D doubles when pref
  BoxLds bL{};
  if constexpr (BOX) {
    static_assert(BOX_MAXIT > 0 && BOX_MAXLS > 0, "compile-time trip bounds");
    bL.Mo = dl;
    bL.bl = bL.Mo + nu * nu;
    bL.bh = bL.bl + nu;
    bL.x = bL.bh + nu;
    bL.gr = bL.x + nu;
    bL.xt = bL.gr + nu;
    bL.xc = bL.xt + nu;
    bL.gc = bL.xc + nu;
    dl = bL.gc + nu;  // box_lds_doubles(nu) further on
  }
  // STD: Qo = luu + B'VB (Mm holds the regularised one, factored in place);
  // lxx, luu: the diagonals 2 (wq, wv), 2 wu of the step's cost row
  double *Qo = nullptr, *lxx = nullptr, *luu = nullptr;
  if constexpr (STD) {
    Qo = dl;
    lxx = Qo + nu * nu;
    luu = lxx + nx;
    dl = luu + nu;  // std_lds_doubles(nv, nu) further on
  }
  // STD: lxx, luu of point p's cost row (of seed s's table: sd.sstride)
  auto hess = [&](int p) {
    if constexpr (STD) {
      const CostDev cr = cost_at(sd.cost, s, sd.sstride, p, sd.cstride);
      for (int i = tid; i < nx; i += BW_THREADS) lxx[i] = 2 * (i < nv ? cr.wq[i] : cr.wv[i - nv]);
      for (int a = tid; a < nu; a += BW_THREADS) luu[a] = 2 * cr.wu[a];
    }
  };
  double dV1 = 0, dV2 = 0;  // STD: the expected reduction's two terms, the same in every lane
  int first_bad = -1;       // STD: the first step that took the fallback
  int* trn = (int*)(dl + (pref ? D : 0));
  double* T4 = A;
  double* Vn = V;
#ifdef ILQG_STAMPS
  unsigned long long bst_prev = 0;
#endif
  // REG: the seed's schedule state (every lane loads the same words)
  double dmu = 1.0;
  int rstatus = 0, retries = 0;
  if constexpr (REG) {
    mu = rg.mu[s];
    dmu = rg.dmu[s];
    rstatus = rg.status[s];
  }

  // initV at the terminal point dArray[0], inc/ilqr.h:100-107
  [[maybe_unused]] restart:
  {
    ready(0);
    const double* q0 = deriv + ((size_t)s * P + 0) * Ds + 2 * nv * nv + nv * nu;
    // v0 = dgdx at the terminal point, or the caller's (an initV override)
    for (int i = tid; i < nx; i += BW_THREADS) v[i] = fl.vinit ? vg[(size_t)s * nx + i] : ld(q0 + i);
    ready(P > 1 ? 1 : 0);
    const double* d1 = deriv + ((size_t)s * P + (P > 1 ? 1 : 0)) * Ds;
    if (pref)
      for (int i = tid; i < D; i += BW_THREADS) dl[i] = ld(d1 + rec_src(i, nv, nu, fl.layout));
    hess(0);
    __syncthreads();
    for (int e = tid; e < nx * nx; e += BW_THREADS) {
      int i = e % nx, j = e / nx;
      if constexpr (STD) V[i + j * LX] = fl.vinit ? Vg[(size_t)s * nx * nx + e] : (i == j ? lxx[i] : 0.0);
      else V[i + j * LX] = fl.vinit ? Vg[(size_t)s * nx * nx + e] : v[i] * v[j];
    }
    __syncthreads();
  }
  BSTAMP(-1);
  // the nominal states for c = x*_{n-1} - x*_n: one lane per component, in
  // registers, each point loaded one step ahead (nq == nv; quaternion models
  // take the tangent-space difference from memory below)
  const bool xreg = !STD && nq == nv && nx <= BW_THREADS;
  auto xload = [&](size_t pt) -> double {
    return tid < nv ? tr.qpos[pt * nq + tid] : (tid < nx ? tr.qvel[pt * nv + tid - nv] : 0.0);
  };
  double xa = 0, xb = 0;
  if (xreg) {
    xa = xload((size_t)s * P);
    if (P > 1) xb = xload((size_t)s * P + 1);
  }
  for (int n = 1; n < P; n++) {
    const size_t pc = (size_t)s * P + n, pp = pc - 1;
    double xn = 0;
    if (xreg && n + 1 < P) xn = xload(pc + 1);
    // prefetch the next step's FD record; consumed at the end of this step
    double pf[BW_PF];
    if (pref && n + 1 < P) {
      ready(n + 1);
      const double* dn1 = deriv + (pc + 1) * Ds;
#pragma unroll
      for (int t = 0; t < BW_PF; t++) {
        int i = tid + t * BW_THREADS;
        pf[t] = i < D ? ld(dn1 + rec_src(i, nv, nu, fl.layout)) : 0.0;
      }
    }
    const double* dn0 = pref ? dl : deriv + pc * Ds;
    // record entry e as the recursion reads it (staged records are already in the layout)
    const int lay = pref ? 0 : fl.layout;
    auto dn = [&](int e) -> double { return dn0[rec_src(e, nv, nu, lay)]; };
    // stage 1: symmetrise V, assemble A/B (differentiator.h:66-71,89-92), q, r, c
    for (int e = tid; e < nx * nx; e += BW_THREADS) {
      int i = e % nx, j = e / nx;
      Vs[i + j * LX] = (V[i + j * LX] + V[j + i * LX]) / 2;
      double val;
      if (i < nv && j < nv) val = (i == j) ? 1 : 0;
      else if (i < nv) val = (i == j - nv) ? dt : 0;
      else if (j < nv) val = dn((i - nv) + j * nv) * dt;
      else val = ((i - nv) == (j - nv) ? 1 : 0) + dn(nv * nv + (i - nv) + (j - nv) * nv) * dt;
      A[i + j * LX] = val;
    }
    for (int e = tid; e < nx * nu; e += BW_THREADS) {
      int i = e % nx, j = e / nx;
      B[i + j * LX] = (i < nv) ? 0 : dn(2 * nv * nv + (i - nv) + j * nv) * dt;
    }
    for (int i = tid; i < nx; i += BW_THREADS) {
      q[i] = dn(2 * nv * nv + nv * nu + i);
      // c = x*_{n-1} (-) x*_n (inc/ilqr.h:154-157; tangent space for quaternion joints)
      if constexpr (STD) {
        // deviation coordinates: no c
      } else if (xreg) {
        c[i] = xa - xb;  // i == tid
      } else if (i < nv && nq != nv) {
        c[i] = dev::state_diff_dof(m, i, tr.qpos + pp * nq, tr.qpos + pc * nq);
      } else {
        double xp = i < nv ? tr.qpos[pp * nq + i] : tr.qvel[pp * nv + i - nv];
        double xc = i < nv ? tr.qpos[pc * nq + i] : tr.qvel[pc * nv + i - nv];
        c[i] = xp - xc;
      }
    }
    for (int a = tid; a < nu; a += BW_THREADS) r[a] = dn(2 * nv * nv + nv * nu + nx + a);
    if constexpr (BOX) {
      // the bounds on this step's feed-forward: lo - u*, hi - u*
      for (int a = tid; a < nu; a += BW_THREADS) {
        const double us = tr.ctrl[pc * nu + a];
        bL.bl[a] = bx.lo[a] - us;
        bL.bh[a] = bx.hi[a] - us;
      }
    }
    hess(n);  // (the step before ended on a barrier behind its last read of lxx, luu)
    __syncthreads();
    if constexpr (!STD) {
      for (int i = tid; i < nx; i += BW_THREADS) Vs[i + i * LX] += mu;
      __syncthreads();
    }
    BSTAMP(0);
    // stage 2: T1 = B'V
    if constexpr (STD) {
      // T1 = B'(V + mu I), the diagonal term added inside the sum; T6 (free
      // until stage 5) takes the unregularised B'V, ld nu
      double* T1u = T6;
      ILP3_BEGIN(nu * nx)
        double s0 = 0, s1 = 0, s2 = 0, u0 = 0, u1 = 0, u2 = 0;
        const int a0 = e0 % nu, j0 = e0 / nu, a1 = f1 % nu, j1 = f1 / nu, a2 = f2 % nu, j2 = f2 / nu;
        for (int kk = 0; kk < nx; kk++) {
          const double b0 = B[kk + a0 * LX], b1 = B[kk + a1 * LX], b2 = B[kk + a2 * LX];
          const double v0 = Vs[kk + j0 * LX], v1 = Vs[kk + j1 * LX], v2 = Vs[kk + j2 * LX];
          u0 += b0 * v0;
          u1 += b1 * v1;
          u2 += b2 * v2;
          s0 += b0 * (kk == j0 ? v0 + mu : v0);
          s1 += b1 * (kk == j1 ? v1 + mu : v1);
          s2 += b2 * (kk == j2 ? v2 + mu : v2);
        }
        T1[e0] = s0;
        T1u[e0] = u0;
        if (h1) T1[e1] = s1, T1u[e1] = u1;
        if (h2) T1[e2] = s2, T1u[e2] = u2;
      }
    } else {
    ILP3_BEGIN(nu * nx)
      double s0 = 0, s1 = 0, s2 = 0;
      const int a0 = e0 % nu, j0 = e0 / nu, a1 = f1 % nu, j1 = f1 / nu, a2 = f2 % nu, j2 = f2 / nu;
      for (int kk = 0; kk < nx; kk++) {
        s0 += B[kk + a0 * LX] * Vs[kk + j0 * LX];
        s1 += B[kk + a1 * LX] * Vs[kk + j1 * LX];
        s2 += B[kk + a2 * LX] * Vs[kk + j2 * LX];
      }
      T1[e0] = s0;
      if (h1) T1[e1] = s1;
      if (h2) T1[e2] = s2;
    }
    }
    __syncthreads();
    BSTAMP(1);
    // stage 3: Mm = -2 T1 B - 2R ; T3 = T1 A ; w = v + 2 V c
    // (STD: Mm = luu + T1 B = Quu_r, Qo = luu + T1u B = Quu ; T3 = Qux_r ; w = v)
    for (int e = tid; e < nu * nu; e += BW_THREADS) {
      int a = e % nu, b = e / nu;
      double sm = 0;
      for (int kk = 0; kk < nx; kk++) sm += T1[a + kk * nu] * B[kk + b * LX];
      if constexpr (STD) {
        double su = 0;
        for (int kk = 0; kk < nx; kk++) su += T6[a + kk * nu] * B[kk + b * LX];
        const double l = a == b ? luu[a] : 0.0;
        Mm[e] = l + sm;
        Qo[e] = l + su;
      } else {
        Mm[e] = -2 * sm - 2 * (r[a] * r[b]);
      }
      if constexpr (BOX) bL.Mo[e] = Mm[e];
    }
    ILP3_BEGIN(nu * nx)
      double s0 = 0, s1 = 0, s2 = 0;
      const int a0 = e0 % nu, j0 = e0 / nu, a1 = f1 % nu, j1 = f1 / nu, a2 = f2 % nu, j2 = f2 / nu;
      for (int kk = 0; kk < nx; kk++) {
        s0 += T1[a0 + kk * nu] * A[kk + j0 * LX];
        s1 += T1[a1 + kk * nu] * A[kk + j1 * LX];
        s2 += T1[a2 + kk * nu] * A[kk + j2 * LX];
      }
      T3[e0] = s0;
      if (h1) T3[e1] = s1;
      if (h2) T3[e2] = s2;
    }
    for (int i = tid; i < nx; i += BW_THREADS) {
      if constexpr (STD) {
        w[i] = v[i];
      } else {
        double sm = 0;
        for (int j = 0; j < nx; j++) sm += Vs[i + j * LX] * c[j];
        w[i] = v[i] + 2 * sm;
      }
    }
    __syncthreads();
    ldlt_factor_wave(nu, Mm, trn, y, tid);  // y is free until stage 5
    for (int a = tid; a < nu; a += BW_THREADS) {
      double sm = 0;
      for (int kk = 0; kk < nx; kk++) sm += B[kk + a * LX] * w[kk];
      col[a] = sm + r[a];
    }
    __syncthreads();
    BSTAMP(2);
    // stage 4: K = ldlt.solve(2 T3) column-parallel; k = ldlt.solve(B'w + r), in place in LDS
    int* perm = trn + nu;
    ldlt_perm(nu, trn, perm, tid);
    for (int j = tid; j < nx + 1; j += BW_THREADS) {
      double* x = j < nx ? Kl + j * nu : kl;
      if (j < nx)
        for (int a = 0; a < nu; a++) x[a] = STD ? -T3[a + j * nu] : 2 * T3[a + j * nu];
      else
        for (int a = 0; a < nu; a++) x[a] = STD ? -col[a] : col[a];
    }
    __syncthreads();
    if (nu <= 32 && nx + 1 <= BW_THREADS) {
      const int j = tid;
      ldlt_solve_reg(nu, Mm, perm, j < nx ? Kl + j * nu : kl, j < nx + 1);
    } else {
      for (int j = tid; j < nx + 1; j += BW_THREADS) ldlt_solve(nu, Mm, trn, j < nx ? Kl + j * nu : kl);
    }
    __syncthreads();
    BSTAMP(3);
    if constexpr (BOX) {
      // fast path: the unconstrained k inside the box (a NaN counts as inside
      // and propagates as in the exact engine) -- K, k stay the exact engine's
      int inside = 1;
      for (int a = 0; a < nu; a++) {
        const double ka = kl[a];
        inside &= (!(ka < bL.bl[a]) && !(ka > bL.bh[a])) ? 1 : 0;
      }
      unsigned cmask = 0, cinfo = 0;
      if (box_uni(!inside)) {
        const unsigned full = nu >= 32 ? ~0u : ((1u << nu) - 1u);
        const int it = box_solve(nu, bL, Mm, col, kl, trn, y, tid, &cmask);  // y is free until stage 5
        if (box_uni(it >= 0)) {
          // K: zero rows for the clamped controls, Mm_ff K_f = (2 T3)_f for the
          // free ones (the final set's factor, its clamped rows isolated)
          cinfo = (unsigned)it;
          if (cmask != full) {
            for (int j = tid; j < nx; j += BW_THREADS) {
              double* xk = Kl + j * nu;
              for (int a = 0; a < nu; a++) xk[a] = ((cmask >> a) & 1u) ? 0.0 : 2 * T3[a + j * nu];
              ldlt_solve(nu, Mm, trn, xk);
              for (int a = 0; a < nu; a++)
                if ((cmask >> a) & 1u) xk[a] = 0.0;
            }
          } else {
            for (int e = tid; e < nu * nx; e += BW_THREADS) Kl[e] = 0.0;
          }
          if (tid < nu) kl[tid] = bL.x[tid];
        } else {
          // fallback: the clipped unconstrained k, zero gain rows where it clipped
          cmask = 0;
          for (int a = 0; a < nu; a++) {
            const double ka = kl[a];
            if (ka < bL.bl[a] || ka > bL.bh[a]) cmask |= 1u << a;
          }
          cmask = (unsigned)box_uni((int)cmask);
          cinfo = 0x80000000u;
          wave_sync();
          for (int e = tid; e < nu * nx; e += BW_THREADS)
            if ((cmask >> (e % nu)) & 1u) Kl[e] = 0.0;
          if (tid < nu) kl[tid] = box_clip(kl[tid], bL.bl[tid], bL.bh[tid]);
        }
        __syncthreads();
      }
      if (tid == 0) {
        bx.mask[pc] = cmask;
        bx.info[pc] = cinfo;
      }
    }
    if constexpr (STD) {
      // Quu_r must be positive definite: every pivot of the factor positive (a
      // NaN fails the comparison).  Otherwise the uncontrolled step.
      int ok = 1;
      for (int a = 0; a < nu; a++) ok &= Mm[a + a * nu] > 0 ? 1 : 0;
      // (and gains that overflowed, from finite records of absurd size, count as indefinite)
      int fin = 1;
      for (int e = tid; e < nu * nx; e += BW_THREADS) fin &= fabs(Kl[e]) <= 1.7976931348623157e308 ? 1 : 0;
      if (tid < nu) fin &= fabs(kl[tid]) <= 1.7976931348623157e308 ? 1 : 0;
      ok &= __ballot(!fin) == 0ull ? 1 : 0;
      if constexpr (REG) {
        // restart at a larger mu: decided from wave-uniform values, taken by every lane
        const int cap = rg.max_retry < REG_MAXRETRY ? rg.max_retry : REG_MAXRETRY;
        if (box_uni(!ok && retries < cap && rstatus == 0)) {
          reg_increase(rg, mu, dmu, rstatus);
          retries++;
          dV1 = 0;
          dV2 = 0;
          first_bad = -1;
          __syncthreads();  // the step's LDS reads are done before initV rewrites V, v, dl
          goto restart;
        }
      }
      if (box_uni(!ok)) {
        if (first_bad < 0) first_bad = n;
        for (int e = tid; e < nu * nx; e += BW_THREADS) Kl[e] = 0.0;
        if (tid < nu) kl[tid] = 0.0;
        __syncthreads();
      } else {
        // every lane the same sums from the same LDS values: col = Qu
        double d1 = 0, d2 = 0;
        for (int a = 0; a < nu; a++) {
          double sm = 0;
          for (int b = 0; b < nu; b++) sm += Qo[a + b * nu] * kl[b];
          d1 += kl[a] * col[a];
          d2 += kl[a] * sm;
        }
        dV1 += d1;
        dV2 += 0.5 * d2;
      }
    }
    // stage 5: ABK = A + B K ; T6 = K'R ; y = Bk + c ; kR = k'R
    // (STD: T6 = K'luu ; y = Bk ; kR = r + luu k)
    for (int e = tid; e < nx * nx; e += BW_THREADS) {
      int i = e % nx, j = e / nx;
      double sm = 0;
      for (int a = 0; a < nu; a++) sm += B[i + a * LX] * Kl[a + j * nu];
      ABK[i + j * LX] = A[i + j * LX] + sm;
    }
    for (int e = tid; e < nx * nu; e += BW_THREADS) {
      int i = e % nx, b = e / nx;
      if constexpr (STD) {
        T6[i + b * LX] = Kl[b + i * nu] * luu[b];
      } else {
        double sm = 0;
        for (int a = 0; a < nu; a++) sm += Kl[a + i * nu] * (r[a] * r[b]);
        T6[i + b * LX] = sm;
      }
    }
    for (int i = tid; i < nx; i += BW_THREADS) {
      double sm = 0;
      for (int a = 0; a < nu; a++) sm += B[i + a * LX] * kl[a];
      if constexpr (STD) y[i] = sm;
      else y[i] = sm + c[i];
    }
    for (int b = tid; b < nu; b += BW_THREADS) {
      if constexpr (STD) {
        kR[b] = r[b] + luu[b] * kl[b];
      } else {
        double sm = 0;
        for (int a = 0; a < nu; a++) sm += kl[a] * (r[a] * r[b]);
        kR[b] = sm;
      }
    }
    __syncthreads();
    BSTAMP(4);
    // stage 6: T4 = ABK' V
    ILP3_BEGIN(nx * nx)
      double s0 = 0, s1 = 0, s2 = 0;
      const int i0 = e0 % nx, j0 = e0 / nx, i1 = f1 % nx, j1 = f1 / nx, i2 = f2 % nx, j2 = f2 / nx;
      for (int kk = 0; kk < nx; kk++) {
        s0 += ABK[kk + i0 * LX] * Vs[kk + j0 * LX];
        s1 += ABK[kk + i1 * LX] * Vs[kk + j1 * LX];
        s2 += ABK[kk + i2 * LX] * Vs[kk + j2 * LX];
      }
      T4[i0 + j0 * LX] = s0;
      if (h1) T4[i1 + j1 * LX] = s1;
      if (h2) T4[i2 + j2 * LX] = s2;
    }
    __syncthreads();
    BSTAMP(5);
    // stage 7: V_new = (T4 ABK + Q) + T6 K
    ILP3_BEGIN(nx * nx)
      double a0s = 0, a1s = 0, a2s = 0, b0s = 0, b1s = 0, b2s = 0;
      const int i0 = e0 % nx, j0 = e0 / nx, i1 = f1 % nx, j1 = f1 / nx, i2 = f2 % nx, j2 = f2 / nx;
      for (int kk = 0; kk < nx; kk++) {
        a0s += T4[i0 + kk * LX] * ABK[kk + j0 * LX];
        a1s += T4[i1 + kk * LX] * ABK[kk + j1 * LX];
        a2s += T4[i2 + kk * LX] * ABK[kk + j2 * LX];
      }
      for (int b = 0; b < nu; b++) {
        b0s += T6[i0 + b * LX] * Kl[b + j0 * nu];
        b1s += T6[i1 + b * LX] * Kl[b + j1 * nu];
        b2s += T6[i2 + b * LX] * Kl[b + j2 * nu];
      }
      if constexpr (STD) {
        Vn[i0 + j0 * LX] = (a0s + (i0 == j0 ? lxx[i0] : 0.0)) + b0s;
        if (h1) Vn[i1 + j1 * LX] = (a1s + (i1 == j1 ? lxx[i1] : 0.0)) + b1s;
        if (h2) Vn[i2 + j2 * LX] = (a2s + (i2 == j2 ? lxx[i2] : 0.0)) + b2s;
      } else {
      Vn[i0 + j0 * LX] = (a0s + q[i0] * q[j0]) + b0s;
      if (h1) Vn[i1 + j1 * LX] = (a1s + q[i1] * q[j1]) + b1s;
      if (h2) Vn[i2 + j2 * LX] = (a2s + q[i2] * q[j2]) + b2s;
      }
    }
    __syncthreads();
    BSTAMP(6);
    if constexpr (STD) {
      // stage 8: z = v + V (B k) (the OLD V, symmetrised) ; v_new = (q + K'kR) + (A+BK)'z
      for (int i = tid; i < nx; i += BW_THREADS) {
        double sm = 0;
        for (int j = 0; j < nx; j++) sm += Vs[i + j * LX] * y[j];
        z[i] = v[i] + sm;
      }
      __syncthreads();
      for (int j = tid; j < nx; j += BW_THREADS) {
        double ta = 0, td = 0;
        for (int i = 0; i < nx; i++) ta += z[i] * ABK[i + j * LX];
        for (int b = 0; b < nu; b++) td += kR[b] * Kl[b + j * nu];
        vn[j] = (q[j] + td) + ta;
      }
    } else {
    // stage 8: z = (2y)' V_new ; v_new (reads the NEW V, Q14)
    for (int j = tid; j < nx; j += BW_THREADS) {
      double sm = 0;
      for (int i = 0; i < nx; i++) sm += (2 * y[i]) * Vn[i + j * LX];
      z[j] = sm;
    }
    __syncthreads();
    for (int j = tid; j < nx; j += BW_THREADS) {
      double ta = 0, tb = 0, td = 0;
      for (int i = 0; i < nx; i++) {
        ta += z[i] * ABK[i + j * LX];
        tb += v[i] * ABK[i + j * LX];
      }
      for (int b = 0; b < nu; b++) td += (2 * kR[b]) * Kl[b + j * nu];
      vn[j] = ((ta + tb) + q[j]) + td;
    }
    }
    BSTAMP(7);
    // gains out
    for (int e = tid; e < nu * nx; e += BW_THREADS) Kg[pc * nu * nx + e] = Kl[e];
    for (int a = tid; a < nu; a += BW_THREADS) kg[pc * nu + a] = kl[a];
    __syncthreads();
    for (int i = tid; i < nx; i += BW_THREADS) v[i] = vn[i];  // V already holds V_new
    if (pref && n + 1 < P) {
#pragma unroll
      for (int t = 0; t < BW_PF; t++) {
        int i = tid + t * BW_THREADS;
        if (i < D) dl[i] = pf[t];
      }
    }
    __syncthreads();
    xa = xb;
    xb = xn;
    BSTAMP(8);
  }
  if (Vg)
    for (int e = tid; e < nx * nx; e += BW_THREADS) {
      int i = e % nx, j = e / nx;
      if constexpr (STD) Vg[(size_t)s * nx * nx + e] = (V[i + j * LX] + V[j + i * LX]) / 2;  // V <- (V + V')/2
      else Vg[(size_t)s * nx * nx + e] = V[i + j * LX];
    }
  if (vg)
    for (int i = tid; i < nx; i += BW_THREADS) vg[(size_t)s * nx + i] = v[i];
  if constexpr (STD) {
    if (tid == 0) {
      sd.dV[2 * (size_t)s] = dV1;
      sd.dV[2 * (size_t)s + 1] = dV2;
      sd.bad[s] = first_bad;
      if constexpr (REG) {
        rg.mu[s] = mu;
        rg.dmu[s] = dmu;
        rg.status[s] = rstatus;
        rg.retries[s] = retries;
        if (rg.trace) {
          rg.trace[(size_t)s * REG_TRACE + 6] = mu;
          rg.trace[(size_t)s * REG_TRACE + 7] = (double)(retries + 100 * rstatus);
        }
      }
    }
  }
}


}  // namespace ilqg
