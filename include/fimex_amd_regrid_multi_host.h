/*
 * fimex_amd_regrid_multi_host.h -- the entries of fimex_amd.h that regrid a list of variables in one call, on host buffers.
 * Same conventions as fimex_amd.h; a header of its own, as fimex_amd_vector_regrid_host.h is.
 */
#ifndef FIMEX_AMD_REGRID_MULTI_HOST_H_
#define FIMEX_AMD_REGRID_MULTI_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_regrid_apply_multi_device on host arrays: in[i] holds nz[i]*inY*inX floats, out[i] has room for nz[i]*outY*outX.
 *  Switches to the plan's device, copies every variable over, copies the results back and synchronises.  The same checks, on
 *  the host addresses; *path as there. */
int fimex_amd_regrid_apply_multi_host(const fimex_amd_regrid_plan* plan, size_t nvar, const float* const* in, const size_t* nz,
                                      float* const* out, int* path);
/** fimex_amd_regrid_apply_multi_typed_device on host arrays of elements of cdmType, in the same way. */
int fimex_amd_regrid_apply_multi_typed_host(const fimex_amd_regrid_plan* plan, size_t nvar, const void* const* in, int cdmType,
                                            const size_t* nz, const double* badValue, void* const* out, int* path);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_REGRID_MULTI_HOST_H_ */
