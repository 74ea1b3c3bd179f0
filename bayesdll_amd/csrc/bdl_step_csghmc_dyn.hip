// bdl_step_csghmc_dyn.hip — the cSGHMC step kernel instances in the dynamic
// sweep order (csg_sweep, bdl_kernels.hpp; include/bdl_order.h) and the drift
// probe's instances.  A translation unit of its own: the static orders'
// instances (bdl_step_csghmc.hip) stay as they are, and the two compile in
// parallel.
#include "bdl_kernels.hpp"

namespace bdl {
namespace {

template <int METHOD, int NOISE, int COLLECT>
DynKernel dyn_unroll(int unroll) {
  switch (unroll) {
    case 1:
      return bdl_step_dyn_kernel<METHOD, NOISE, COLLECT, 1>;
    case 4:
      return bdl_step_dyn_kernel<METHOD, NOISE, COLLECT, 4>;
    default:
      return bdl_step_dyn_kernel<METHOD, NOISE, COLLECT, 2>;
  }
}

template <int METHOD, int NOISE>
DynKernel dyn_collect(int collect, int unroll) {
  switch (collect) {
    case BDL_COLLECT_NONE:
      return dyn_unroll<METHOD, NOISE, BDL_COLLECT_NONE>(unroll);
    case BDL_COLLECT_WELFORD_INIT:
      return dyn_unroll<METHOD, NOISE, BDL_COLLECT_WELFORD_INIT>(unroll);
    case BDL_COLLECT_WELFORD:
      return dyn_unroll<METHOD, NOISE, BDL_COLLECT_WELFORD>(unroll);
    case BDL_COLLECT_MEAN_INIT:
      return dyn_unroll<METHOD, NOISE, BDL_COLLECT_MEAN_INIT>(unroll);
    case BDL_COLLECT_MEAN:
      return dyn_unroll<METHOD, NOISE, BDL_COLLECT_MEAN>(unroll);
  }
  return nullptr;
}

}  // namespace

DynKernel pick_step_csghmc_dyn(int noise, int collect, int unroll, bool bare) {
  if (bare) return dyn_collect<kMethodBare, BDL_NOISE_NONE>(collect, unroll);
  switch (noise) {
    case BDL_NOISE_NONE:
      return dyn_collect<BDL_CSGHMC, BDL_NOISE_NONE>(collect, unroll);
    case BDL_NOISE_BUFFER:
      return dyn_collect<BDL_CSGHMC, BDL_NOISE_BUFFER>(collect, unroll);
    case BDL_NOISE_PHILOX:
      return dyn_collect<BDL_CSGHMC, BDL_NOISE_PHILOX>(collect, unroll);
  }
  return nullptr;
}

DriftKernel pick_drift(int unroll, bool dyn) {
  switch (unroll) {
    case 1:
      return dyn ? bdl_drift_kernel<1, true> : bdl_drift_kernel<1, false>;
    case 4:
      return dyn ? bdl_drift_kernel<4, true> : bdl_drift_kernel<4, false>;
    default:
      return dyn ? bdl_drift_kernel<2, true> : bdl_drift_kernel<2, false>;
  }
}

}  // namespace bdl
