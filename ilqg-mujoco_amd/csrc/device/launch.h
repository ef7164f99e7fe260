// Host side of every hot-path launch: the LDS opt-in, the typed launch and
// the choice of the generic kernels' model type.  (A header of its own, which
// coop_common.h includes: kernels_fd32.hip launches through it too, and that
// unit cannot take coop_common.h's fp64 names beside its fp32 ones.)
#pragma once
#include <cstdlib>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "dmodel.h"

namespace ilqg {

// more than 64 KB of dynamic LDS has to be allowed per kernel
template <typename K>
hipError_t allow_lds(K kern, size_t lds) {
  if (lds <= 65536) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds);
}

// allow_lds -> launch -> hipGetLastError.  The kernel's parameter types are the
// arguments' own (references and cv dropped): `kern` may name a template with a
// trailing parameter pack (k_fd_centre_s<SM, SX, SCH...>), whose instance the
// arguments then select, and a list that is not exactly the kernel's does not
// compile.
template <class... A>
hipError_t launch(void (*kern)(std::type_identity_t<A>...), unsigned blocks, unsigned threads, size_t lds,
                  hipStream_t st, const A&... a) {
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, st, a...);
  return hipGetLastError();
}

// The model type MT of the generic kernels that take one (k_rollout2_coop,
// k_fd_centre32, k_fd_cols32): NV<27> (DevModelNV of the unit's physics
// instance) for 27-dof models, the humanoid, else DevModel; ILQG_NV_CONST=0
// keeps DevModel (A/B).  f(std::type_identity<MT>{}) makes the launch.
template <template <int> class NV, class F>
hipError_t for_model_type(const DevModel& m, F&& f) {
  static const int nvc_env = [] {
    const char* v = getenv("ILQG_NV_CONST");
    return (v && v[0] == '0') ? 0 : 1;
  }();
  if (nvc_env && m.nv == 27) return f(std::type_identity<NV<27>>{});
  return f(std::type_identity<DevModel>{});
}

}  // namespace ilqg
