// The LEVELS InvMgmt policy kernels (INVSIM_POLICY_LEVELS): invmgmt.hip compiled
// again with INVSIM_IM_LVL_TU, where every policy kernel (im_run_kernel,
// im_roll3o_kernel, im_roll3_kernel, both demand streams) orders up to the
// env's own levels from the attached device arrays, and which defines
// im_lvl_launch.  As for invmgmt_rnd.hip the variant is a macro and not a
// template argument, so the other objects hold the kernels they held before.
#define INVSIM_IM_LVL_TU
#include "invmgmt.hip"
