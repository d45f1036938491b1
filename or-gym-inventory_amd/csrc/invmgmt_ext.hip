// The EXTERNAL InvMgmt run kernels (invsim_rollout_metrics): invmgmt.hip
// compiled again with INVSIM_IM_EXT_TU, which selects im_ext_launch as the
// launcher this object defines, and with it the EXT instantiations of
// im_run_kernel of both demand streams: the policy bookkeeping (metrics,
// optional outputs) with each step's orders from the caller's action rows.
// An object of its own, as invmgmt_rnd.hip.  Only im_run_kernel is emitted
// here: the launcher names no other kernel, and a template that is not
// instantiated emits nothing.
#define INVSIM_IM_EXT_TU
#include "invmgmt.hip"
