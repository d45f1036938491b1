// Fast-stream (PhiloxGen) InvMgmt kernels: invmgmt.hip compiled again with
// INVSIM_IM_FAST_TU, which selects im_run_launch_ph as the launcher this
// object defines, and with it the PhiloxGen instantiations of the step, run
// and rollout kernels (the parity stream's stay in invmgmt.o; see the end of
// invmgmt.hip).
#define INVSIM_IM_FAST_TU
#include "invmgmt.hip"
