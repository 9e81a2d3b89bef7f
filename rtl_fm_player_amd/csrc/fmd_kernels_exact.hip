/* The EX instantiations of fmd_fused_kernel (FMD_MATH_EXACT) and their launcher: one of three translation units over fmd_kernels.inc, split by
 * instantiation set so that they compile in parallel (same flags for all three, see Makefile). */
#define FMD_BUILD_EXACT 1
#include "fmd_kernels.inc"
