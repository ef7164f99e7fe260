// The rollout of one (seed, alpha) candidate (inc/ilqr.h:116-130), the default
// kernels around it and their launcher, shared by the rollout kernels' two
// translation units: kernels_rollout.hip and, for the
// cost-schedule variants, kernels_rollout_sch.hip (every instance inlines the
// whole physics step: one unit would take twice as long to compile).
#pragma once
//
// The rollout's Newton solves use the model's tolerance, and their line
// searches take ~1.4 iterations: the uniform-row line search (dcoop_impl.h
// ls_iterate_rows, for the FD sweep's tolerance-0 solves) does not pay here,
// and its code grew the hopper rollout kernel from 240 to 299 KB, slowing
// every stage (instruction cache): this translation unit keeps the lane form
// for the iterations of the generic solver, and runs the compile-time models'
// line searches (eval(0) included) on rows padded to 4 or 8 (linesearch_u).
#ifndef ILQG_LS_NE
#define ILQG_LS_NE 0
#endif
#ifndef ILQG_LS_U
#define ILQG_LS_U 1
#endif
// (~1.4 iterations per line search: the speculative bisection tree does not pay)
#ifndef ILQG_LS_TREE
#define ILQG_LS_TREE 0
#endif
// (the Newton loops' replay exit, dcoop_impl.h: a frozen iteration ends these
// solves on improvement < tol already, and the kernel is sensitive to code size)
#ifndef ILQG_NT_REPLAY
#define ILQG_NT_REPLAY 0
#endif
#include "coop_common.h"

namespace ilqg {

// kernels_rollout_sch.hip: launch_rollout_coop's launch while a cost schedule
// is set (a.cstride != 0), clamped to the control limits or not
hipError_t launch_rollout_sch(const DevModel& m, const WsLayout& L, const coop::CoopLayout& C,
                              const coop::CoopAux& X, const RollArgs& a, bool lim);

namespace {

__device__ inline void rollout_body(const auto& m, const auto& L, const auto& C, const auto& X, const Team& T,
                                int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch, int wave, auto split, auto lowreg, auto clamp, auto sched, int cstride = 0, int sstride = 0) {
  // clamp (the kernels' LIM instances, launched while control limits are set):
  // the control law's output confined to [ch.ulim[i], ch.ulim[nu + i]]
  // sched (their <.., int, int> instances, launched while a cost schedule is set):
  // point n is charged with row n of the seed's schedule, cost.wq + s sstride +
  // n cstride (sstride = 0: one table for every seed), which is packed as
  // stage_cost lays the LDS copy out (wq tq lq wv tv lv wu tu lu)
  // wave < 0: one-wave team; 0/1: primary/helper wave of a two-wave team (step_dual)
  const bool prim = wave <= 0;
  STAMP_INIT();
#ifdef ILQG_STAMPS
  unsigned long long rt0 = __builtin_amdgcn_s_memrealtime(), mt0 = __builtin_amdgcn_s_memtime();
#endif
  const int lane = blockIdx.x;
  const int s = lane / A, a = lane % A;
  const int nq = m.nq, nv = m.nv, nu = m.nu, nx = 2 * nv;
  // the points this launch rolls over (RollChunk): n_hi .. n_lo, descending
  const int nhi = ch.n_hi >= 0 ? ch.n_hi : P - 1, nlo = ch.n_hi >= 0 ? ch.n_lo : 0;
  const bool resume = nhi < P - 1;
  if (resume) load_state(m, L, T, ch.carry, lane, s, qfrc_applied, xfrc_applied);
  else load_state(m, L, T, dinit, s, s, qfrc_applied, xfrc_applied);
  // (a resumed chunk of a scheduled rollout stages row n_hi, not row 0)
  constexpr bool SCH = decltype(sched)::value;
  if constexpr (SCH) cost = cost_at(cost, s, sstride);  // the seed's table (cost.wq: its row 0)
  const CostDev cl = stage_cost(m, C, T, [&] {
    if constexpr (SCH) return cost_at(cost, nhi, cstride);
    else return cost;
  }());
  double* qpos = T.w + L.qpos;
  double* qvel = T.w + L.qvel;
  double* ctrl = T.w + L.ctrl;
  double* warm = T.w + L.warm;
  double* dx = T.w + L.s_fd;
  // per-point record of the nominal trajectory and gains, [x*_q | x*_v | u* | K | k],
  // prefetched one point ahead into registers and parked in LDS (C.rec)
  double* rec = T.c + C.rec;
  const int R = nq + nv + nu + nu * nx + nu;
  // ch.dbuf (generic two-wave kernel): point n's record in buffer (nhi - n) & 1,
  // the second one past the team's LDS (launch_rollout_coop sized the launch)
  double* rec2 = rec;
  if (ch.dbuf) {
    extern __shared__ double lds[];
    const size_t off = ((size_t)(L.nd + C.nd + C.imgd) * 8 + (size_t)(L.ni + C.ni) * 4 + 15) / 16 * 16;
    rec2 = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + off);
  }
  auto recp = [&](int n) -> double* { return ((nhi - n) & 1) ? rec2 : rec; };
  auto fetch = [&](size_t pn, int t) -> double {
    if (t < nq) return nom.qpos[pn * nq + t];
    t -= nq;
    if (t < nv) return nom.qvel[pn * nv + t];
    t -= nv;
    if (t < nu) return nom.ctrl[pn * nu + t];
    t -= nu;
    if (t < nu * nx) return K[pn * nu * nx + t];
    return k[pn * nu + t - nu * nx];
  };
  // registers per lane: R <= PFR * 64.  The run-time (generic) models take
  // records up to 20 * 64 doubles (the humanoid's is 1231: K alone is
  // nu x 2nv = 1134) in flight a step ahead as well
  using MT = std::remove_cvref_t<decltype(m)>;
  // (lowreg: the two-wave generic kernel, whose record is double-buffered in LDS
  // instead -- 20 prefetch registers spilled to scratch there, a 512-register kernel)
  constexpr int PFR = StaticModel<MT> ? 4 : (decltype(lowreg)::value ? 1 : 20);
  double pf[PFR];
  // larger records are not prefetched: park() copies them from global memory directly
  const bool pfok = R <= PFR * TEAM_SIZE;
  // sched: the next point's cost row, CN doubles, prefetched beside the record
  // (the humanoid's 228 doubles: 4 per lane); longer rows are copied directly
  [[maybe_unused]] const int CN = 3 * (nq + nv + nu);
  constexpr int CPF = [] {
    if constexpr (StaticModel<MT>) return (3 * (MT::nq + MT::nv + MT::nu) + TEAM_SIZE - 1) / TEAM_SIZE;
    else return 4;
  }();
  [[maybe_unused]] const bool cpok = CN <= CPF * TEAM_SIZE;
  if (!passive) {
    FOR_T(t, R) rec[t] = fetch((size_t)s * P + nhi, t);
    TSYNC();
  }
  const double alpha = alphas ? alphas[a] : 1.0;
  const int ob = out_is_cand ? lane : s;
  // the wave that runs the control law and writes the record: the helper wave
  // of a two-wave team (beside the primary's kinematics), else the only wave
  const bool ctl = wave < 0 || wave == 1;
  double c = 0;
  if (resume && ctl && T.tid == 0 && cost_cand) c = cost_cand[lane];
  // control law u = u* + alpha k + K (x - x*) for point n, its record and cost
  // (ilqr.h:116-133); the next point's nominal record is prefetched first
  auto pre_step = [&](int n) {
    const double* rq = recp(n);
    const double* rv = rq + nq;
    const double* ru = rq + nq + nv;
    const double* rK = ru + nu;
    const double* rk = rK + nu * nx;
    const bool pre = !passive && n > 0 && pfok && !ch.dbuf;
    [[maybe_unused]] double cpf[CPF];
    if constexpr (SCH) {
      if (n > nlo && cpok) {
        const double* row = cost.wq + (size_t)(n - 1) * (size_t)cstride;
#pragma unroll
        for (int q = 0; q < CPF; q++) {
          const int t = T.tid + q * TEAM_SIZE;
          cpf[q] = t < CN ? row[t] : 0.0;
        }
      }
    }
    if (pre) {
      const size_t pn1 = (size_t)s * P + (n - 1);
#pragma unroll
      for (int q = 0; q < PFR; q++) {
        const int t = T.tid + q * TEAM_SIZE;
        pf[q] = t < R ? fetch(pn1, t) : 0.0;
      }
    }
    if (!passive) {
      FOR_T(j, nx) dx[j] = j < nv ? state_diff_dof(m, j, qpos, rq) : qvel[j - nv] - rv[j - nv];
      TSYNC();
      FOR_T(i, nu) {
        double t = 0;
        int j = 0;
        if constexpr (!StaticModel<MT>) {
          // run-time nx: eight terms' loads in flight at once, additions in order
          for (; j + 8 <= nx; j += 8) {
            double kk[8], xx[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
              kk[q] = rK[i + (j + q) * nu];
              xx[q] = dx[j + q];
            }
#pragma unroll
            for (int q = 0; q < 8; q++) t += kk[q] * xx[q];
          }
        }
        for (; j < nx; j++) t += rK[i + j * nu] * dx[j];
        double cv = (t + alpha * rk[i]) + ru[i];
        if constexpr (decltype(clamp)::value) {
          // (+-0 and NaN pass through unchanged); the record and the cost take the clamped value
          const double lo = ch.ulim[i], hi = ch.ulim[nu + i];
          cv = cv < lo ? lo : (cv > hi ? hi : cv);
        }
        ctrl[i] = cv;
      }
      TSYNC();
    }
    const size_t po = (size_t)ob * P + n;
    FOR_T(i, nq) out.qpos[po * nq + i] = qpos[i];
    FOR_T(i, nv) {
      out.qvel[po * nv + i] = qvel[i];
      out.warm[po * nv + i] = warm[i];
    }
    FOR_T(i, nu) out.ctrl[po * nu + i] = ctrl[i];
    if (T.tid == 0) {
      out.time[po] = T.w[L.time];
      c += step_cost(m, cl, qpos, qvel, ctrl);
    }
    TSYNC();
    if constexpr (SCH) {
      // row n - 1 replaces row n in the LDS copy once lane 0 has charged point n:
      // this wave alone reads and writes the copy after stage_cost
      if (n > nlo) {
        double* cd = T.c + C.cdesc;
        if (cpok) {
#pragma unroll
          for (int q = 0; q < CPF; q++) {
            const int t = T.tid + q * TEAM_SIZE;
            if (t < CN) cd[t] = cpf[q];
          }
        } else {
          const double* row = cost.wq + (size_t)(n - 1) * (size_t)cstride;
          FOR_T(t, CN) cd[t] = row[t];
        }
        TSYNC();
      }
    }
  };
  // the prefetched record replaces the current one once the step no longer reads it
  auto park = [&](int n) {
    if (!passive && n > 0 && !ch.dbuf) {
      if (pfok) {
#pragma unroll
        for (int q = 0; q < PFR; q++) {
          const int t = T.tid + q * TEAM_SIZE;
          if (t < R) rec[t] = pf[q];
        }
      } else {
        FOR_T(t, R) rec[t] = fetch((size_t)s * P + (n - 1), t);
      }
      TSYNC();
    }
  };
  if (wave >= 0) {
    // the step ids of the two-wave hand-off flags (step_dual_split) start above 0
    if (threadIdx.x == 0)
      T.ci[C.ibc + 1] = T.ci[C.ibc + 2] = T.ci[C.ibc + 3] = T.ci[C.ibc + 4] = T.ci[C.ibc + 6] = T.ci[C.ibc + 7] = 0;
    __syncthreads();
  }
  for (int n = nhi; n >= nlo; n--) {
    if (wave < 0) {
      pre_step(n);
      step(m, L, C, X, T);
      park(n);
    } else {
      // split layout (compile-time models): the rebalanced three-wave
      // schedule, which parks the record in a later phase
      if constexpr (decltype(split)::value) {
        step_dual_split(m, L, C, X, T, wave, P - n, [&]() { pre_step(n); }, [&]() { park(n); });
      } else {
        step_dual(
            m, L, C, X, T, wave,
            [&]() {
              pre_step(n);
              park(n);
            },
            [&]() {
              // the next point's record into the other buffer (ch.dbuf)
              if (ch.dbuf && !passive && n > 0) {
                double* dst = recp(n - 1);
                const size_t pn1 = (size_t)s * P + (n - 1);
                for (int t0 = T.tid; t0 < R; t0 += 4 * TEAM_SIZE) {
                  double v[4];
#pragma unroll
                  for (int q = 0; q < 4; q++) {
                    const int t = t0 + q * TEAM_SIZE;
                    v[q] = t < R ? fetch(pn1, t) : 0.0;
                  }
#pragma unroll
                  for (int q = 0; q < 4; q++)
                    if (t0 + q * TEAM_SIZE < R) dst[t0 + q * TEAM_SIZE] = v[q];
                }
              }
            });
      }
    }
  }
  if (ctl && T.tid == 0 && cost_cand) cost_cand[lane] = c;
  if (nlo > 0) {
    // the state the next chunk starts from (point nlo - 1, before its control)
    if (wave >= 0) __syncthreads();
    if (prim) {
      FOR_T(i, nq) ch.carry.qpos[(size_t)lane * nq + i] = qpos[i];
      FOR_T(i, nv) {
        ch.carry.qvel[(size_t)lane * nv + i] = qvel[i];
        ch.carry.warm[(size_t)lane * nv + i] = warm[i];
      }
      FOR_T(i, nu) ch.carry.ctrl[(size_t)lane * nu + i] = ctrl[i];
      if (T.tid == 0) ch.carry.time[lane] = T.w[L.time];
    }
  }
#ifdef ILQG_STAMPS
  if (prim && T.tid == 0 && blockIdx.x == 0) {
    g_stamp_acc[46] += __builtin_amdgcn_s_memrealtime() - rt0;
    g_stamp_acc[47] += __builtin_amdgcn_s_memtime() - mt0;
  }
#endif
  STAMP_FLUSH();
}

// three-wave teams for the compile-time register-row models (step_dual_split),
// two-wave otherwise
template <class SM>
constexpr int rollout_waves() { return SM::nv <= RMAX ? 3 : 2; }

// LDS a rollout workgroup reserves: its workspace, or (ILQG_ROLLOUT_LDS) more,
// so that no FD team can share its CU
inline size_t rollout_lds(size_t need) {
  static long pad = -1;
  if (pad < 0) {
    const char* e = getenv("ILQG_ROLLOUT_LDS");
    pad = e ? atol(e) : 0;
  }
  return (size_t)pad > need ? (size_t)pad : need;
}

// ---- the default rollout kernels.  LIM: the control law clamped to the
// solver's control limits (RollChunk.ulim); SCH...: a cost schedule's two
// strides (coop_common.h).  Each unit instantiates the ones it launches.
// two-wave teams (step_dual): 128 threads per (seed, candidate).  MT: DevModel,
// or DevModelNV<27> for 27-dof models (the humanoid: compile-time sizes in the
// Newton Cholesky and its substitution)
template <class MT, bool LIM, class... SCH>
__global__ __launch_bounds__(2 * TEAM) void k_rollout2_coop(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch, SCH... cstride) {
  Team T = make_team(L, C);
  MT m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::false_type{}, std::true_type{},
               std::bool_constant<LIM>{}, std::bool_constant<(sizeof...(SCH) > 0)>{}, sched_stride(cstride...), sched_seed(cstride...));
}
// three-wave teams for the compile-time register-row models (rollout_waves)
template <class SM, class SX, bool LIM, class... SCH>
__global__ __launch_bounds__(3 * TEAM) void k_rollout2_s(DevModel mg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch, SCH... cstride) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair, true);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::bool_constant<SM::nv <= RMAX>{},
               std::false_type{}, std::bool_constant<LIM>{}, std::bool_constant<(sizeof...(SCH) > 0)>{},
               sched_stride(cstride...), sched_seed(cstride...));
}

// the second buffer of the generic kernel's record, past the workspace when it
// fits (RollChunk.dbuf; ILQG_ROLL_DBUF=0 keeps the register prefetch, A/B):
// sets ch.dbuf and returns the launch's LDS
inline size_t rollout_dbuf_lds(const DevModel& m, const WsLayout& L, const CoopLayout& C, size_t lds, RollChunk& ch) {
  static const int dbuf_env = [] {
    const char* v = getenv("ILQG_ROLL_DBUF");
    return (v && v[0] == '0') ? 0 : 1;
  }();
  const size_t R = (size_t)m.nq + m.nv + m.nu + (size_t)m.nu * 2 * m.nv + m.nu;
  const size_t need = (coop_lds_bytes(L, C) + 15) / 16 * 16 + R * sizeof(double);
  if (dbuf_env && need <= 160 * 1024) {
    ch.dbuf = 1;
    return need > lds ? need : lds;
  }
  return lds;
}

// launch of the default kernels: the bundled model's k_rollout2_s, or
// k_rollout2_coop; cs... is the cost schedule's strides (SCH = int, int) or empty
template <bool LIM, class... SCH>
hipError_t launch_rollout2(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                           const RollArgs& a, SCH... cs) {
  const unsigned blocks = a.S * a.A;
  hipError_t e = hipSuccess;
  if (for_static_model(m.static_id, [&](auto sm, auto sx) {
        using SM = decltype(sm);
        using SX = decltype(sx);
        const size_t lds2 = rollout_lds(coop_lds_bytes(make_layout(sm, SX::npair, true), C));
        e = launch(k_rollout2_s<SM, SX, LIM, SCH...>, blocks, rollout_waves<SM>() * TEAM, lds2, a.st, m, a.S, a.A, a.P,
                   a.nominal, a.out, a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied, a.xfrc_applied,
                   a.passive, a.cost, a.cost_cand, a.ch, cs...);
      }))
    return e;
  RollChunk ch = a.ch;
  const size_t lds_d = rollout_dbuf_lds(m, L, C, rollout_lds(coop_lds_bytes(L, C)), ch);
  return for_model_type<DevModelNV>(m, [&](auto mt) {
    return launch(k_rollout2_coop<typename decltype(mt)::type, LIM, SCH...>, blocks, 2 * TEAM, lds_d, a.st, m, L, C, X,
                  a.S, a.A, a.P, a.nominal, a.out, a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied,
                  a.xfrc_applied, a.passive, a.cost, a.cost_cand, ch, cs...);
  });
}

}  // namespace
}  // namespace ilqg
