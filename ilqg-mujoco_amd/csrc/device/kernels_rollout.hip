// Cooperative rollout kernels (inc/ilqr.h:116-130): one workgroup per
// (seed, alpha) candidate; two-wave teams (step_dual) by default.  The variants
// that charge a cost schedule are in kernels_rollout_sch.hip.
#include "rollout_body.h"

namespace ilqg {
namespace {

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

// two-wave teams (step_dual): 128 threads per (seed, candidate).  MT: DevModel,
// or DevModelNV<27> for 27-dof models (the humanoid: compile-time sizes in the
// Newton Cholesky and its substitution)
template <class MT>
__global__ __launch_bounds__(2 * TEAM) void k_rollout2_coop(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  Team T = make_team(L, C);
  MT m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::false_type{}, std::true_type{},
               std::false_type{}, std::false_type{});
}
// k_rollout2_coop with the control law clamped to the solver's control limits (RollChunk.ulim)
template <class MT>
__global__ __launch_bounds__(2 * TEAM) void k_rollout2_coop_lim(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  Team T = make_team(L, C);
  MT m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::false_type{}, std::true_type{},
               std::true_type{}, std::false_type{});
}
// three-wave teams for the compile-time register-row models (rollout_waves)
template <class SM, class SX>
__global__ __launch_bounds__(3 * TEAM) void k_rollout2_s(DevModel mg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair, true);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::bool_constant<SM::nv <= RMAX>{},
               std::false_type{}, std::false_type{}, std::false_type{});
}
// k_rollout2_s with the control law clamped to the solver's control limits (RollChunk.ulim)
template <class SM, class SX>
__global__ __launch_bounds__(3 * TEAM) void k_rollout2_s_lim(DevModel mg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair, true);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::bool_constant<SM::nv <= RMAX>{},
               std::false_type{}, std::true_type{}, std::false_type{});
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

}  // namespace

static bool use_dual() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("ILQG_DUAL");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}
hipError_t launch_rollout_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X, int S,
                               int A, int P, TrajDev nominal, TrajDev out, int out_is_cand, const double* K,
                               const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied,
                               const double* xfrc_applied, int passive, CostDev cost, double* cost_cand,
                               hipStream_t st, RollChunk ch, int cstride) {
  const size_t lds = rollout_lds(coop_lds_bytes(L, C));
  hipError_t e;
  // control limits: the clamped variants of the default kernels (k_rollout2_s,
  // k_rollout2_coop); the passive constructor rollout has no control law
  const bool lim = ch.ulim != nullptr && !passive;
  if (lim && !use_dual()) return hipErrorNotSupported;
  // cost schedule: the scheduled variants of the same kernels, clamped or not
  const bool sch = cstride != 0 && !passive;
  if (sch && !use_dual()) return hipErrorNotSupported;
  const RollArgs ra{S, A, P, nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost,
                    cost_cand, st, ch, cstride};
  if (sch) {
    bool done = false;
    e = launch_rollout_sch_static(m, C, ra, lim, done);
    if (done) return e;
  } else if (lim) {
#define ILQG_CASE(id, SMT, SXT)                                                                                 \
  case id: {                                                                                                    \
    const size_t lds2 = rollout_lds(coop_lds_bytes(make_layout(stat::SMT{}, stat::SXT::npair, true), C));       \
    e = allow_lds(k_rollout2_s_lim<stat::SMT, stat::SXT>, lds2);                                                \
    if (e != hipSuccess) return e;                                                                              \
    hipLaunchKernelGGL((k_rollout2_s_lim<stat::SMT, stat::SXT>), dim3(S * A),                                   \
                       dim3(rollout_waves<stat::SMT>() * TEAM), lds2, st, m, S, A, P,                            \
                       nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, \
                       cost_cand, ch);                                                                              \
    return hipGetLastError();                                                                                   \
  }
    switch (m.static_id) {
      ILQG_STATIC_MODELS(ILQG_CASE)
      default:
        break;
    }
#undef ILQG_CASE
  }
  if (use_dual()) {
#define ILQG_CASE(id, SMT, SXT)                                                                                 \
  case id: {                                                                                                    \
    const size_t lds2 = rollout_lds(coop_lds_bytes(make_layout(stat::SMT{}, stat::SXT::npair, true), C));       \
    e = allow_lds(k_rollout2_s<stat::SMT, stat::SXT>, lds2);                                                    \
    if (e != hipSuccess) return e;                                                                              \
    hipLaunchKernelGGL((k_rollout2_s<stat::SMT, stat::SXT>), dim3(S * A),                                       \
                       dim3(rollout_waves<stat::SMT>() * TEAM), lds2, st, m, S, A, P,                            \
                       nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, \
                       cost_cand, ch);                                                                              \
    return hipGetLastError();                                                                                   \
  }
    switch (m.static_id) {
      ILQG_STATIC_MODELS(ILQG_CASE)
      default:
        break;
    }
#undef ILQG_CASE
    // the record's second buffer past the workspace when it fits (RollChunk.dbuf;
    // ILQG_ROLL_DBUF=0 keeps the register prefetch, A/B)
    size_t lds_d = lds;
    {
      static const int dbuf_env = [] {
        const char* v = getenv("ILQG_ROLL_DBUF");
        return (v && v[0] == '0') ? 0 : 1;
      }();
      const size_t R = (size_t)m.nq + m.nv + m.nu + (size_t)m.nu * 2 * m.nv + m.nu;
      const size_t need = (coop_lds_bytes(L, C) + 15) / 16 * 16 + R * sizeof(double);
      if (dbuf_env && need <= 160 * 1024) {
        ch.dbuf = 1;
        lds_d = need > lds ? need : lds;
      }
    }
    static const int nvc_env = [] {
      const char* v = getenv("ILQG_NV_CONST");
      return (v && v[0] == '0') ? 0 : 1;
    }();
    const bool nv27 = nvc_env && m.nv == 27;
    const void* kf = nv27 ? reinterpret_cast<const void*>(k_rollout2_coop<DevModelNV<27>>)
                          : reinterpret_cast<const void*>(k_rollout2_coop<DevModel>);
    e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);
    if (e != hipSuccess) return e;
    if (sch) {
      RollArgs rd = ra;
      rd.ch = ch;  // (dbuf set above)
      return launch_rollout_sch_generic(m, L, C, X, rd, lim, nv27, lds_d);
    }
    if (lim) {
      const void* kl = nv27 ? reinterpret_cast<const void*>(k_rollout2_coop_lim<DevModelNV<27>>)
                            : reinterpret_cast<const void*>(k_rollout2_coop_lim<DevModel>);
      e = hipFuncSetAttribute(kl, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d);
      if (e != hipSuccess) return e;
      if (nv27)
        hipLaunchKernelGGL(k_rollout2_coop_lim<DevModelNV<27>>, dim3(S * A), dim3(2 * TEAM), lds_d, st, m, L, C, X, S,
                           A, P, nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive,
                           cost, cost_cand, ch);
      else
        hipLaunchKernelGGL(k_rollout2_coop_lim<DevModel>, dim3(S * A), dim3(2 * TEAM), lds_d, st, m, L, C, X, S, A, P,
                           nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost,
                           cost_cand, ch);
      return hipGetLastError();
    }
    if (nv27)
      hipLaunchKernelGGL(k_rollout2_coop<DevModelNV<27>>, dim3(S * A), dim3(2 * TEAM), lds_d, st, m, L, C, X, S, A,
                         P, nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost,
                         cost_cand, ch);
    else
    hipLaunchKernelGGL(k_rollout2_coop<DevModel>, dim3(S * A), dim3(2 * TEAM), lds_d, st, m, L, C, X, S, A, P, nominal, out,
                       out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, cost_cand, ch);
    return hipGetLastError();
  }
#define ILQG_CASE(id, SMT, SXT)                                                                                 \
  case id:                                                                                                      \
    e = allow_lds(k_rollout_s<stat::SMT, stat::SXT>, lds);                                                      \
    if (e != hipSuccess) return e;                                                                              \
    hipLaunchKernelGGL((k_rollout_s<stat::SMT, stat::SXT>), dim3(S * A), dim3(TEAM), lds, st, m, S, A, P,        \
                       nominal, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, \
                       cost_cand, ch);                                                                              \
    return hipGetLastError();
  switch (m.static_id) {
    ILQG_STATIC_MODELS(ILQG_CASE)
    default:
      break;
  }
#undef ILQG_CASE
  e = allow_lds(k_rollout_coop, coop_lds_bytes(L, C));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rollout_coop, dim3(S * A), dim3(TEAM), coop_lds_bytes(L, C), st, m, L, C, X, S, A, P, nominal,
                     out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied, passive, cost, cost_cand, ch);
  return hipGetLastError();
}

bool rollout_clamp_supported() { return use_dual(); }
bool rollout_sched_supported() { return use_dual(); }

hipError_t launch_select(const DevModel& m, int S, int A, int P, int mode, int copy_cand, const double* cost_cand,
                         int* sel, double* cost_sel, TrajDev cand, TrajDev nominal, TrajDev dinit, hipStream_t st) {
  hipLaunchKernelGGL(k_select, dim3(S), dim3(256), 0, st, m.nq, m.nv, m.nu, S, A, P, mode, copy_cand, cost_cand,
                     sel, cost_sel, cand, nominal, dinit);
  return hipGetLastError();
}

hipError_t launch_step_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                            TrajDev stt, int n, int nstep, const double* qfrc_applied, const double* xfrc_applied,
                            hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e;
#define ILQG_CASE(id, SMT, SXT)                                                                                  \
  case id: {                                                                                                     \
    const size_t lds = coop_lds_bytes(make_layout(stat::SMT{}, stat::SXT::npair), C);                           \
    e = allow_lds(k_step_s<stat::SMT, stat::SXT>, lds);                                                          \
    if (e != hipSuccess) return e;                                                                               \
    hipLaunchKernelGGL((k_step_s<stat::SMT, stat::SXT>), dim3(n), dim3(TEAM), lds, st, m, stt, nstep,           \
                       qfrc_applied, xfrc_applied);                                                              \
    return hipGetLastError();                                                                                    \
  }
  switch (m.static_id) {
    ILQG_STATIC_MODELS(ILQG_CASE)
    default:
      break;
  }
#undef ILQG_CASE
  e = allow_lds(k_step_coop, coop_lds_bytes(L, C));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_step_coop, dim3(n), dim3(TEAM), coop_lds_bytes(L, C), st, m, L, C, X, stt, nstep,
                     qfrc_applied, xfrc_applied);
  return hipGetLastError();
}

hipError_t launch_forward_coop(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                               TrajDev stt, int n, const double* qfrc_applied, const double* xfrc_applied,
                               double* qacc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e;
#define ILQG_CASE(id, SMT, SXT)                                                                                  \
  case id: {                                                                                                     \
    const size_t lds = coop_lds_bytes(make_layout(stat::SMT{}, stat::SXT::npair), C);                           \
    e = allow_lds(k_fwd_s<stat::SMT, stat::SXT>, lds);                                                           \
    if (e != hipSuccess) return e;                                                                               \
    hipLaunchKernelGGL((k_fwd_s<stat::SMT, stat::SXT>), dim3(n), dim3(TEAM), lds, st, m, stt, qfrc_applied,     \
                       xfrc_applied, qacc);                                                                      \
    return hipGetLastError();                                                                                    \
  }
  switch (m.static_id) {
    ILQG_STATIC_MODELS(ILQG_CASE)
    default:
      break;
  }
#undef ILQG_CASE
  e = allow_lds(k_fwd_coop, coop_lds_bytes(L, C));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fwd_coop, dim3(n), dim3(TEAM), coop_lds_bytes(L, C), st, m, L, C, X, stt, qfrc_applied,
                     xfrc_applied, qacc);
  return hipGetLastError();
}

}  // namespace ilqg

#ifdef ILQG_STAMPS
// the rollout kernels' line-search counters (dcoop_impl.h g_ls)
extern "C" int ilqg_debug_ls_rollout(unsigned long long* out5, int reset) {
  if (hipMemcpyFromSymbol(out5, HIP_SYMBOL(ilqg::coop::g_ls), sizeof(unsigned long long) * 8) != hipSuccess) return 3;
  if (reset) {
    unsigned long long z[8] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ilqg::coop::g_ls), z, sizeof(z));
  }
  return 0;
}
extern "C" int ilqg_debug_stamps(unsigned long long* acc, unsigned long long* cnt, int reset) {
  if (hipMemcpyFromSymbol(acc, HIP_SYMBOL(ilqg::coop::g_stamp_acc), sizeof(unsigned long long) * STAMP_NG) != hipSuccess)
    return 3;
  if (hipMemcpyFromSymbol(cnt, HIP_SYMBOL(ilqg::coop::g_stamp_cnt), sizeof(unsigned long long) * STAMP_NG) != hipSuccess)
    return 3;
  unsigned long long nw[2];
  (void)hipMemcpyFromSymbol(&nw[0], HIP_SYMBOL(ilqg::coop::g_newton_iters), 8);
  (void)hipMemcpyFromSymbol(&nw[1], HIP_SYMBOL(ilqg::coop::g_newton_calls), 8);
  acc[44] = nw[0];
  acc[45] = nw[1];
  if (reset) {
    unsigned long long z[STAMP_NG] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ilqg::coop::g_newton_iters), z, 8);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ilqg::coop::g_newton_calls), z, 8);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ilqg::coop::g_stamp_acc), z, sizeof(z));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ilqg::coop::g_stamp_cnt), z, sizeof(z));
  }
  return 0;
}
#endif
