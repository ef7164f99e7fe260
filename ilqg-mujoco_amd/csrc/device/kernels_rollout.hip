// Cooperative rollout kernels (inc/ilqr.h:116-130): one workgroup per
// (seed, alpha) candidate; two-wave teams (step_dual) by default: k_rollout2_s
// and k_rollout2_coop (rollout_body.h), whose instances without a cost schedule
// this unit launches; kernels_rollout_sch.hip launches the scheduled ones.
#include "rollout_body.h"

namespace ilqg {
namespace {

// one-wave teams (ILQG_DUAL=0)
__global__ __launch_bounds__(TEAM) void k_rollout_coop(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  Team T = make_team(L, C);
  DevModel m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, cost_cand, ch, -1, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
}

// model-specific instance (static_models.h): compile-time sizes, tables and LDS layout
template <class SM, class SX>
__global__ __launch_bounds__(TEAM) void k_rollout_s(DevModel mg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, cost_cand, ch, -1, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{});
}

// ---- batch physics (ilqg_step_batch / ilqg_forward_batch): one wavefront per state
// mj_step x nstep from each state (cpMjData in, the state out)
__device__ inline void step_batch_body(const auto& m, const auto& L, const auto& C, const auto& X, const Team& T,
                                       TrajDev stt, int nstep, const double* qfrc_applied, const double* xfrc_applied) {
  const int i = blockIdx.x;
  load_state(m, L, T, stt, i, i, qfrc_applied, xfrc_applied);
  for (int t = 0; t < nstep; t++) step(m, L, C, X, T);
  if (T.tid == 0) stt.time[i] = T.w[L.time];
  FOR_T(k, m.nq) stt.qpos[(size_t)i * m.nq + k] = T.w[L.qpos + k];
  FOR_T(k, m.nv) {
    stt.qvel[(size_t)i * m.nv + k] = T.w[L.qvel + k];
    stt.warm[(size_t)i * m.nv + k] = T.w[L.warm + k];
  }
}
// mj_forward at each state: qacc out, qacc_warmstart updated in place
__device__ inline void fwd_batch_body(const auto& m, const auto& L, const auto& C, const auto& X, const Team& T,
                                      TrajDev stt, const double* qfrc_applied, const double* xfrc_applied,
                                      double* qacc) {
  const int i = blockIdx.x;
  load_state(m, L, T, stt, i, i, qfrc_applied, xfrc_applied);
  forward_skip(m, L, C, X, T, STAGE_NONE, m.opt_iterations, m.opt_tolerance);
  FOR_T(k, m.nv) {
    qacc[(size_t)i * m.nv + k] = T.w[L.qacc + k];
    stt.warm[(size_t)i * m.nv + k] = T.w[L.warm + k];
  }
}
__global__ __launch_bounds__(TEAM) void k_step_coop(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, TrajDev stt,
                                                    int nstep, const double* qfrc_applied, const double* xfrc_applied) {
  Team T = make_team(L, C);
  DevModel m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  step_batch_body(m, L, C, X, T, stt, nstep, qfrc_applied, xfrc_applied);
}
template <class SM, class SX>
__global__ __launch_bounds__(TEAM) void k_step_s(DevModel mg, TrajDev stt, int nstep, const double* qfrc_applied,
                                                 const double* xfrc_applied) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  step_batch_body(m, L, C, X, T, stt, nstep, qfrc_applied, xfrc_applied);
}
__global__ __launch_bounds__(TEAM) void k_fwd_coop(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, TrajDev stt,
                                                   const double* qfrc_applied, const double* xfrc_applied,
                                                   double* qacc) {
  Team T = make_team(L, C);
  DevModel m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  fwd_batch_body(m, L, C, X, T, stt, qfrc_applied, xfrc_applied, qacc);
}
template <class SM, class SX>
__global__ __launch_bounds__(TEAM) void k_fwd_s(DevModel mg, TrajDev stt, const double* qfrc_applied,
                                                const double* xfrc_applied, double* qacc) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  fwd_batch_body(m, L, C, X, T, stt, qfrc_applied, xfrc_applied, qacc);
}

// line-search selection + setDInit (inc/ilqr.h:110-113): per seed, the
// candidate with the smallest trajectory cost (mode 1; a NaN cost never wins
// over a number) or alpha = 1 (mode 0), copied to the nominal trajectory
__global__ void k_select(int nq, int nv, int nu, int S, int A, int P, int mode, int copy_cand,
                         const double* cost_cand, int* sel, double* cost_sel, TrajDev cand, TrajDev nom,
                         TrajDev dinit) {
  int s = blockIdx.x;
  __shared__ int best_sh;
  if (threadIdx.x == 0) {
    int best = 0;
    if (mode == 1 && cost_cand) {
      double bc = cost_cand[(size_t)s * A];
      for (int a = 1; a < A; a++) {
        double c = cost_cand[(size_t)s * A + a];
        if (c < bc || (bc != bc && c == c)) { bc = c; best = a; }
      }
    }
    best_sh = best;
    if (sel) sel[s] = best;
    if (cost_sel && cost_cand) cost_sel[s] = cost_cand[(size_t)s * A + best];
  }
  __syncthreads();
  int best = best_sh;
  if (copy_cand) {
    size_t src0 = ((size_t)s * A + best) * P, dst0 = (size_t)s * P;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
      nom.time[dst0 + p] = cand.time[src0 + p];
      for (int i = 0; i < nq; i++) nom.qpos[(dst0 + p) * nq + i] = cand.qpos[(src0 + p) * nq + i];
      for (int i = 0; i < nv; i++) nom.qvel[(dst0 + p) * nv + i] = cand.qvel[(src0 + p) * nv + i];
      for (int i = 0; i < nv; i++) nom.warm[(dst0 + p) * nv + i] = cand.warm[(src0 + p) * nv + i];
      for (int i = 0; i < nu; i++) nom.ctrl[(dst0 + p) * nu + i] = cand.ctrl[(src0 + p) * nu + i];
    }
  }
  __syncthreads();
  // setDInit(dArray[N]), inc/ilqr.h:183
  if (threadIdx.x == 0) {
    size_t src = (size_t)s * P + (P - 1);
    const TrajDev& t = copy_cand ? cand : nom;
    size_t sp = copy_cand ? ((size_t)s * A + best) * P + (P - 1) : src;
    dinit.time[s] = t.time[sp];
    for (int i = 0; i < nq; i++) dinit.qpos[(size_t)s * nq + i] = t.qpos[sp * nq + i];
    for (int i = 0; i < nv; i++) dinit.qvel[(size_t)s * nv + i] = t.qvel[sp * nv + i];
    for (int i = 0; i < nv; i++) dinit.warm[(size_t)s * nv + i] = t.warm[sp * nv + i];
    for (int i = 0; i < nu; i++) dinit.ctrl[(size_t)s * nu + i] = t.ctrl[sp * nu + i];
  }
}

// k_select's place in the regularisation mode (RegDev, kernels.h), one block
// per seed.  With a valid nominal cost, candidate a is acceptable when
//   actual = cost_nom - cost[a] > 0  and  actual >= zmin * expected,
//   expected = -(alpha_a dV1 + alpha_a alpha_a dV2)
// (a NaN fails both): mode 1 takes the acceptable candidate of lowest cost (a
// tie: the lower index), mode 0 tests candidate 0 alone.  Accepted: the
// candidate becomes the nominal trajectory and dinit, cost_nom and cost_sel
// its cost, mu is lowered, status 1 once actual < tol_cost.  Rejected: nothing
// is copied, cost_sel keeps the nominal's cost, sel = -1, mu is raised.  A seed
// whose status is not 0 rejects everything and keeps its mu.  Without a valid
// nominal cost the choice is k_select's, unconditionally, and mu stays.
__global__ void k_accept(int nq, int nv, int nu, int S, int A, int P, int mode, const double* cost_cand,
                         const double* alphas, const double* dV, int* sel, double* cost_sel, TrajDev cand,
                         TrajDev nom, TrajDev dinit, RegDev rg) {
  const int s = blockIdx.x;
  __shared__ int pick_sh;
  if (threadIdx.x == 0) {
    const double* cc = cost_cand + (size_t)s * A;
    // k_select's choice
    int best = 0;
    if (mode == 1) {
      double bc = cc[0];
      for (int a = 1; a < A; a++) {
        const double c = cc[a];
        if (c < bc || (bc != bc && c == c)) { bc = c; best = a; }
      }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double mu = rg.mu[s], dmu = rg.dmu[s];
    int status = rg.status[s];
    const double mu_before = mu, cn = rg.cost_nom[s], dV1 = dV[2 * (size_t)s], dV2 = dV[2 * (size_t)s + 1];
    auto expected = [&](int a) { return -(alphas[a] * dV1 + alphas[a] * alphas[a] * dV2); };
    int pick = -1;
    double t0 = nan, t3 = nan;
    if (!rg.valid[s]) {
      pick = best;
      rg.valid[s] = 1;
    } else {
      t0 = cn;
      t3 = expected(best);
      if (status == 0) {
        double pc = 0;
        for (int a = 0; a < (mode == 1 ? A : 1); a++) {
          const double actual = cn - cc[a];
          if (actual > 0 && actual >= rg.zmin * expected(a) && (pick < 0 || cc[a] < pc)) {
            pick = a;
            pc = cc[a];
          }
        }
        if (pick >= 0) {
          t3 = expected(pick);
          reg_decrease(rg, mu, dmu);
          if (cn - cc[pick] < rg.tol_cost) status = 1;
        } else {
          reg_increase(rg, mu, dmu, status);
        }
      }
    }
    if (pick >= 0) {
      rg.cost_nom[s] = cc[pick];
      cost_sel[s] = cc[pick];
    }
    sel[s] = pick;
    rg.mu[s] = mu;
    rg.dmu[s] = dmu;
    rg.status[s] = status;
    if (rg.trace) {
      double* t = rg.trace + (size_t)s * REG_TRACE;
      t[0] = t0;
      t[1] = cc[best];
      t[2] = (double)pick;
      t[3] = t3;
      t[4] = mu_before;
      t[5] = mu;
      // (6, 7: the backward pass that follows)
      t[6] = nan;
      t[7] = nan;
    }
    pick_sh = pick;
  }
  __syncthreads();
  const int pick = pick_sh;
  if (pick < 0) return;
  const size_t src0 = ((size_t)s * A + pick) * P, dst0 = (size_t)s * P;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    nom.time[dst0 + p] = cand.time[src0 + p];
    for (int i = 0; i < nq; i++) nom.qpos[(dst0 + p) * nq + i] = cand.qpos[(src0 + p) * nq + i];
    for (int i = 0; i < nv; i++) nom.qvel[(dst0 + p) * nv + i] = cand.qvel[(src0 + p) * nv + i];
    for (int i = 0; i < nv; i++) nom.warm[(dst0 + p) * nv + i] = cand.warm[(src0 + p) * nv + i];
    for (int i = 0; i < nu; i++) nom.ctrl[(dst0 + p) * nu + i] = cand.ctrl[(src0 + p) * nu + i];
  }
  // setDInit(dArray[N]), inc/ilqr.h:183
  if (threadIdx.x == 0) {
    const size_t sp = src0 + (P - 1);
    dinit.time[s] = cand.time[sp];
    for (int i = 0; i < nq; i++) dinit.qpos[(size_t)s * nq + i] = cand.qpos[sp * nq + i];
    for (int i = 0; i < nv; i++) dinit.qvel[(size_t)s * nv + i] = cand.qvel[sp * nv + i];
    for (int i = 0; i < nv; i++) dinit.warm[(size_t)s * nv + i] = cand.warm[sp * nv + i];
    for (int i = 0; i < nu; i++) dinit.ctrl[(size_t)s * nu + i] = cand.ctrl[sp * nu + i];
  }
}

}  // namespace

static bool use_dual() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("ILQG_DUAL");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}
hipError_t launch_rollout_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                               const RollArgs& a) {
  // control limits: the clamped instances of the default kernels (k_rollout2_s,
  // k_rollout2_coop); the passive constructor rollout has no control law
  const bool lim = a.ch.ulim != nullptr && !a.passive;
  if (lim && !use_dual()) return hipErrorNotSupported;
  // cost schedule: the scheduled instances of the same kernels, clamped or not
  const bool sch = a.cstride != 0 && !a.passive;
  if (sch && !use_dual()) return hipErrorNotSupported;
  if (sch) return launch_rollout_sch(m, L, C, X, a, lim);
  if (use_dual()) return lim ? launch_rollout2<true>(m, L, C, X, a) : launch_rollout2<false>(m, L, C, X, a);
  // ILQG_DUAL=0: the one-wave kernels
  const unsigned blocks = a.S * a.A;
  hipError_t e = hipSuccess;
  if (for_static_model(m.static_id, [&](auto sm, auto sx) {
        e = launch(k_rollout_s<decltype(sm), decltype(sx)>, blocks, TEAM, rollout_lds(coop_lds_bytes(L, C)), a.st, m,
                   a.S, a.A, a.P, a.nominal, a.out, a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied,
                   a.xfrc_applied, a.passive, a.cost, a.cost_cand, a.ch);
      }))
    return e;
  return launch(k_rollout_coop, blocks, TEAM, coop_lds_bytes(L, C), a.st, m, L, C, X, a.S, a.A, a.P, a.nominal, a.out,
                a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied, a.xfrc_applied, a.passive, a.cost,
                a.cost_cand, a.ch);
}

bool rollout_clamp_supported() { return use_dual(); }
bool rollout_sched_supported() { return use_dual(); }

hipError_t launch_select(const DevModel& m, int S, int A, int P, int mode, int copy_cand, const double* cost_cand,
                         int* sel, double* cost_sel, TrajDev cand, TrajDev nominal, TrajDev dinit, hipStream_t st) {
  hipLaunchKernelGGL(k_select, dim3(S), dim3(256), 0, st, m.nq, m.nv, m.nu, S, A, P, mode, copy_cand, cost_cand,
                     sel, cost_sel, cand, nominal, dinit);
  return hipGetLastError();
}

hipError_t launch_accept(const DevModel& m, int S, int A, int P, int mode, const double* cost_cand,
                         const double* alphas, const double* dV, int* sel, double* cost_sel, TrajDev cand,
                         TrajDev nominal, TrajDev dinit, RegDev rg, hipStream_t st) {
  if (!cost_cand || !alphas || !dV || !sel || !cost_sel || !cand.qpos || cand.qpos == nominal.qpos || !rg.mu ||
      !rg.dmu || !rg.cost_nom || !rg.valid || !rg.status)
    return hipErrorInvalidValue;
  return launch(k_accept, (unsigned)S, 256u, 0, st, m.nq, m.nv, m.nu, S, A, P, mode, cost_cand, alphas, dV, sel,
                cost_sel, cand, nominal, dinit, rg);
}

hipError_t launch_step_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                            TrajDev stt, int n, int nstep, const double* qfrc_applied, const double* xfrc_applied,
                            hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipSuccess;
  if (for_static_model(m.static_id, [&](auto sm, auto sx) {
        const size_t lds = coop_lds_bytes(make_layout(sm, decltype(sx)::npair), C);
        e = launch(k_step_s<decltype(sm), decltype(sx)>, n, TEAM, lds, st, m, stt, nstep, qfrc_applied, xfrc_applied);
      }))
    return e;
  return launch(k_step_coop, n, TEAM, coop_lds_bytes(L, C), st, m, L, C, X, stt, nstep, qfrc_applied, xfrc_applied);
}

hipError_t launch_forward_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                               TrajDev stt, int n, const double* qfrc_applied, const double* xfrc_applied,
                               double* qacc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipSuccess;
  if (for_static_model(m.static_id, [&](auto sm, auto sx) {
        const size_t lds = coop_lds_bytes(make_layout(sm, decltype(sx)::npair), C);
        e = launch(k_fwd_s<decltype(sm), decltype(sx)>, n, TEAM, lds, st, m, stt, qfrc_applied, xfrc_applied, qacc);
      }))
    return e;
  return launch(k_fwd_coop, n, TEAM, coop_lds_bytes(L, C), st, m, L, C, X, stt, qfrc_applied, xfrc_applied, qacc);
}

}  // namespace ilqg

#ifdef ILQG_STAMPS
// the rollout kernels' copy of the line-search and stamp counters (coop_common.h)
extern "C" int ilqg_debug_ls_rollout(unsigned long long* out5, int reset) { return ilqg::debug_ls(out5, reset); }
extern "C" int ilqg_debug_stamps(unsigned long long* acc, unsigned long long* cnt, int reset) {
  return ilqg::debug_stamps(acc, cnt, reset);
}
#endif
