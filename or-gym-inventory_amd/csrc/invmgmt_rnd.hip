// The RANDOM (RandomAgent) InvMgmt policy kernels: invmgmt.hip compiled again
// with INVSIM_IM_RND_TU, which selects im_rnd_launch as the launcher this
// object defines, and with it the RND instantiations of im_run_kernel,
// im_roll3o_kernel and im_roll3_kernel of both demand streams (the variant is
// a template argument; see the end of invmgmt.hip).  An object of its own, so
// that invmgmt.o and invmgmt_ph.o hold the kernels they held before RANDOM
// existed.
#define INVSIM_IM_RND_TU
#include "invmgmt.hip"
