/*
 * fimex_amd_merge_vector_host.h -- the merge of an x/y vector pair (fimex_amd_merge_apply_vector_device of fimex_amd.h) on host
 * buffers.  Same conventions as fimex_amd.h; a header of its own, as the other late *_host entries have.
 */
#ifndef FIMEX_AMD_MERGE_VECTOR_HOST_H_
#define FIMEX_AMD_MERGE_VECTOR_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_merge_apply_vector_device on host arrays: copies the four fields over, copies the two results back and synchronises;
 *  switches to the plans' device for the call.  The same checks, on the host addresses. */
int fimex_amd_merge_apply_vector_host(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                      const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                      const float* innerU, const float* innerV, const float* outerU, const float* outerV, size_t nz, float* outU,
                                      float* outV);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_MERGE_VECTOR_HOST_H_ */
