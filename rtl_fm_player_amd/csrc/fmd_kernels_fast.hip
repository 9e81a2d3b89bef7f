/* The vector-ALU +-1 LSB instantiations (MX = 0, FMD_MATH_FAST_VALU), fmdk_launch, which picks the unit of a variant, and the tiling helpers:
 * one of three translation units over fmd_kernels.inc, split by instantiation set so that they compile in parallel (same flags, see Makefile). */
#define FMD_BUILD_EXACT 0
#include "fmd_kernels.inc"
