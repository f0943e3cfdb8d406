/*
 * fimex_amd_vector_regrid_typed_host.h -- the entry of the vector block of fimex_amd.h that regrids and rotates a vector pair in
 * its stored types on host buffers.  Same conventions as fimex_amd.h; a header of its own, as fimex_amd_vector_regrid_host.h is.
 */
#ifndef FIMEX_AMD_VECTOR_REGRID_TYPED_HOST_H_
#define FIMEX_AMD_VECTOR_REGRID_TYPED_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_regrid_apply_vector_typed_device on host arrays: u, v hold size = nz*inY*inX elements of uType / vType each (a
 *  remainder is ignored, as CachedInterpolation.cc:121 does), uOut, vOut room for outCapacity >= nz*outY*outX elements of the same
 *  types each; *newSize = nz*outY*outX.  Switches to the plan's device, copies both components over in their stored types,
 *  copies both results back in their stored types and synchronises.  The same checks. */
int fimex_amd_regrid_apply_vector_typed_host(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec,
                                             const void* u, int uType, double uBad,
                                             const void* v, int vType, double vBad, size_t size,
                                             void* uOut, void* vOut, size_t outCapacity, size_t* newSize);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_VECTOR_REGRID_TYPED_HOST_H_ */
