/* The matrix-pipe instantiations (MX = 1 and 2: FMD_MATH_FAST_MFMA, FMD_MATH_FAST_MFMA_F) and their launcher: one of three translation units over
 * fmd_kernels.inc, split by instantiation set so that they compile in parallel (same flags, see Makefile). */
#define FMD_BUILD_EXACT 0
#define FMD_BUILD_MFMA 1
#include "fmd_kernels.inc"
