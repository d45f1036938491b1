// The RANDOM (RandomAgent) InvMgmt policy kernels: invmgmt.hip compiled again
// with INVSIM_IM_RND_TU, where every policy kernel is the variant that draws
// its orders from the env's action generator (im_run_kernel, im_roll3o_kernel,
// im_roll3_kernel, both demand streams), and which defines im_rnd_launch.  The
// variant is this macro and not a template argument so that invmgmt.hip
// without it is unchanged text: invmgmt.o and invmgmt_ph.o then hold the
// kernels they held before RANDOM existed.
#define INVSIM_IM_RND_TU
#include "invmgmt.hip"
