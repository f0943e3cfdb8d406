/*
 * fimex_amd_vector_regrid_host.h -- the entry of the vector block of fimex_amd.h that regrids and rotates a vector pair on host
 * buffers.  Same conventions as fimex_amd.h; a header of its own, as fimex_amd_extract_host.h is.
 */
#ifndef FIMEX_AMD_VECTOR_REGRID_HOST_H_
#define FIMEX_AMD_VECTOR_REGRID_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_regrid_apply_vector_device on host arrays: u, v hold size = nz*inY*inX floats each (a remainder is ignored, as
 *  CachedInterpolation.cc:121 does), uOut, vOut room for outCapacity >= nz*outY*outX floats each; *newSize = nz*outY*outX.
 *  Switches to the plan's device, copies both components over, copies both results back and synchronises.  The same checks. */
int fimex_amd_regrid_apply_vector_host(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec,
                                       const float* u, const float* v, size_t size,
                                       float* uOut, float* vOut, size_t outCapacity, size_t* newSize);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_VECTOR_REGRID_HOST_H_ */
