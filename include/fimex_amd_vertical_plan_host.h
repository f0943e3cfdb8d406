/*
 * fimex_amd_vertical_plan_host.h -- the entries of the vertical plan block (8f n5b) of fimex_amd.h that work on host buffers.
 * Same conventions as fimex_amd.h; a header of its own, as fimex_amd_extract_host.h is.
 */
#ifndef FIMEX_AMD_VERTICAL_PLAN_HOST_H_
#define FIMEX_AMD_VERTICAL_PLAN_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_vertical_plan_create_device with ps / field of the two level descriptions, validMin and validMax on the host: they
 *  are copied over, the plan is built on the calling thread's device and the call synchronises.  The same checks. */
int fimex_amd_vertical_plan_create_host(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                                        const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo,
                                        const double* validMin, const double* validMax, fimex_amd_vertical_plan** plan);

/** fimex_amd_vertical_plan_apply_device on host variables: in[] and out[] hold host pointers; switches to the plan's device,
 *  copies every variable over, copies the results back and synchronises.  The same checks. */
int fimex_amd_vertical_plan_apply_host(const fimex_amd_vertical_plan* plan, size_t nvar, const void* const* in, int cdmType,
                                       const double* badValue, const float* clampMin, const float* clampMax, void* const* out);

/** The decoded entries [nt][nzo][ny][nx] on the host, for tests and diagnostics: the pair of input levels and the folded factor.
 *  Undefined entries come back with first == second.  Waits for the build. */
int fimex_amd_vertical_plan_read_host(const fimex_amd_vertical_plan* plan, unsigned* first, unsigned* second, float* factor);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_VERTICAL_PLAN_HOST_H_ */
