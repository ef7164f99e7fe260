// The rollout kernels of a solver with a cost schedule
// (ilqg_solver_set_cost_schedule): the <.., int, int> instances of k_rollout2_s and
// k_rollout2_coop (rollout_body.h) -- point n charged with row n of the
// schedule, the LDS cost copy re-staged per point from a row prefetched into
// registers -- each with and without the control-limit clamp.  A unit of its
// own beside kernels_rollout.hip for build time: every instance inlines the
// whole physics step.
#include "rollout_body.h"

namespace ilqg {

hipError_t launch_rollout_sch(const DevModel& m, const WsLayout& L, const CoopLayout& C, const CoopAux& X,
                              const RollArgs& a, bool lim) {
  return lim ? launch_rollout2<true>(m, L, C, X, a, a.cstride, a.sstride)
             : launch_rollout2<false>(m, L, C, X, a, a.cstride, a.sstride);
}

}  // namespace ilqg
