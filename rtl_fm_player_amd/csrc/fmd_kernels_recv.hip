/* The receivers beside the batch: kernels of their own, in a translation unit of their own.  They share nothing with the fused kernel
 * (fmd_kernels.inc and its three units) but the memory layouts named below and FMDK_TILE of fmd_internal.h, and reference nothing of the host
 * layer.  Same flags as the fused units (Makefile: -ffp-contract=off, no SLP vectoriser) - the receivers' bit-exact tests rest on them.
 *   levels.inc      the finish kernel of a levels / squelch launch
 *   spectrum.inc    the capture spectrum: a kernel of its own over the same d_iq layout
 *   subcarrier.inc  the MPX subcarrier receiver: kernels of their own over the layout of the `v` debug tap
 *   rds.inc         the RDS receiver: kernels of their own over the subcarrier receiver's z
 *   tuner.inc       the channel tuner: a down-converter of its own over the d_iq layout, u8 in and u8 out
 *   scan.inc        the station finder: a kernel of its own over the layout the capture spectrum writes
 *   stereo.inc      stereo control: pilot meter, tracker and PCM blend, kernels of their own over the PCM the fused kernel wrote */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstddef>
#include <type_traits>

#include "fmd_internal.h"

#include "levels.inc"
#include "spectrum.inc"
#include "subcarrier.inc"
#include "rds.inc"
#include "tuner.inc"
#include "scan.inc"
#include "stereo.inc"
