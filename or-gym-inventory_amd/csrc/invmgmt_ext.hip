// The EXTERNAL InvMgmt run kernels (invsim_rollout_metrics): invmgmt.hip
// compiled again with INVSIM_IM_EXT_TU, where im_run_kernel's policy
// instantiations keep the policy bookkeeping (metrics, optional outputs) but
// take each step's orders from the caller's action rows, and which defines
// im_ext_launch.  As for invmgmt_rnd.hip the variant is a macro and not a
// template argument, so invmgmt.o, invmgmt_ph.o and invmgmt_rnd.o hold the
// kernels they held before.  Only im_run_kernel is emitted here: the split
// step and the fused rollout kernels are guarded out of this translation unit.
#define INVSIM_IM_EXT_TU
#include "invmgmt.hip"
