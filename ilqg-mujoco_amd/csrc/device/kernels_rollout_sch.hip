// The rollout kernels of a solver with a cost schedule
// (ilqg_solver_set_cost_schedule): k_rollout2_s and k_rollout2_coop with
// rollout_body's `sched` tag -- point n charged with row n of the schedule, the
// LDS cost copy re-staged per point from a row prefetched into registers --
// each with and without the control-limit clamp.  launch_rollout_coop
// (kernels_rollout.hip) hands its launch over when cstride != 0; the stride is
// the kernels' last argument.
#include "rollout_body.h"

namespace ilqg {
namespace {

// k_rollout2_coop with a cost schedule (row stride cstride), LIM: clamped as k_rollout2_coop_lim
template <class MT, bool LIM>
__global__ __launch_bounds__(2 * TEAM) void k_rollout2_coop_sch(DevModel mg, WsLayout L, CoopLayout C, CoopAux Xg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch, int cstride) {
  Team T = make_team(L, C);
  MT m;
  CoopAux X;
  stage_model(mg, Xg, L, C, T, m, X);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::false_type{}, std::true_type{},
               std::bool_constant<LIM>{}, std::true_type{}, cstride);
}
// k_rollout2_s with a cost schedule (row stride cstride), LIM: clamped as k_rollout2_s_lim
template <class SM, class SX, bool LIM>
__global__ __launch_bounds__(3 * TEAM) void k_rollout2_s_sch(DevModel mg, int S, int A, int P, TrajDev nom, TrajDev out, int out_is_cand, const double* K, const double* k, const double* alphas, TrajDev dinit, const double* qfrc_applied, const double* xfrc_applied, int passive, CostDev cost, double* cost_cand, RollChunk ch, int cstride) {
  static constexpr WsLayout L = make_layout(SM{}, SX::npair, true);
  static constexpr CoopLayout C = make_coop_layout(SM{}, SX::npair);
  static constexpr SX X{};
  Team T = make_team(L, C);
  SM m;
  stage_model_sep(mg, T, m);
  rollout_body(m, L, C, X, T, S, A, P, nom, out, out_is_cand, K, k, alphas, dinit, qfrc_applied, xfrc_applied,
               passive, cost, cost_cand, ch, (int)(threadIdx.x / TEAM), std::bool_constant<SM::nv <= RMAX>{},
               std::false_type{}, std::bool_constant<LIM>{}, std::true_type{}, cstride);
}

template <class KT>
hipError_t launch_static(KT kern, unsigned threads, size_t lds, const DevModel& m, const RollArgs& a) {
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.S * a.A), dim3(threads), lds, a.st, m, a.S, a.A, a.P, a.nominal, a.out,
                     a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied, a.xfrc_applied, a.passive, a.cost,
                     a.cost_cand, a.ch, a.cstride);
  return hipGetLastError();
}
template <class KT>
hipError_t launch_generic(KT kern, size_t lds, const DevModel& m, const WsLayout& L, const CoopLayout& C,
                          const CoopAux& X, const RollArgs& a) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.S * a.A), dim3(2 * TEAM), lds, a.st, m, L, C, X, a.S, a.A, a.P, a.nominal, a.out,
                     a.out_is_cand, a.K, a.k, a.alphas, a.dinit, a.qfrc_applied, a.xfrc_applied, a.passive, a.cost,
                     a.cost_cand, a.ch, a.cstride);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rollout_sch_static(const DevModel& m, const CoopLayout& C, const RollArgs& a, bool lim,
                                     bool& done) {
  done = true;
#define ILQG_CASE(id, SMT, SXT)                                                                                 \
  case id: {                                                                                                    \
    const size_t lds2 = rollout_lds(coop_lds_bytes(make_layout(stat::SMT{}, stat::SXT::npair, true), C));       \
    const unsigned nt = rollout_waves<stat::SMT>() * TEAM;                                                      \
    return lim ? launch_static(k_rollout2_s_sch<stat::SMT, stat::SXT, true>, nt, lds2, m, a)                    \
               : launch_static(k_rollout2_s_sch<stat::SMT, stat::SXT, false>, nt, lds2, m, a);                  \
  }
  switch (m.static_id) {
    ILQG_STATIC_MODELS(ILQG_CASE)
    default:
      break;
  }
#undef ILQG_CASE
  done = false;
  return hipSuccess;
}

hipError_t launch_rollout_sch_generic(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                                      const RollArgs& a, bool lim, bool nv27, size_t lds_d) {
  if (nv27)
    return lim ? launch_generic(k_rollout2_coop_sch<DevModelNV<27>, true>, lds_d, m, L, C, X, a)
               : launch_generic(k_rollout2_coop_sch<DevModelNV<27>, false>, lds_d, m, L, C, X, a);
  return lim ? launch_generic(k_rollout2_coop_sch<DevModel, true>, lds_d, m, L, C, X, a)
             : launch_generic(k_rollout2_coop_sch<DevModel, false>, lds_d, m, L, C, X, a);
}

}  // namespace ilqg
