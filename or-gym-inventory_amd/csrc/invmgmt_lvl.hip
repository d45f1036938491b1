// The LEVELS InvMgmt policy kernels (INVSIM_POLICY_LEVELS): invmgmt.hip compiled
// again with INVSIM_IM_LVL_TU, which selects im_lvl_launch as the launcher this
// object defines, and with it the LVL instantiations of im_run_kernel,
// im_roll3o_kernel and im_roll3_kernel of both demand streams, which order up
// to the env's own levels from the attached device arrays.  An object of its
// own, as invmgmt_rnd.hip, so the other objects hold the kernels they held
// before.
#define INVSIM_IM_LVL_TU
#include "invmgmt.hip"
