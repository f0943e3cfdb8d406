/*
 * fimex_amd_merge_vector_typed_host.h -- the merge of an x/y vector pair in its stored types
 * (fimex_amd_merge_apply_vector_typed_device of fimex_amd.h) on host buffers.  Same conventions as fimex_amd.h; a header of its
 * own, as the other late *_host entries have.
 */
#ifndef FIMEX_AMD_MERGE_VECTOR_TYPED_HOST_H_
#define FIMEX_AMD_MERGE_VECTOR_TYPED_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_merge_apply_vector_typed_device on host arrays: copies the four fields over in their stored types, copies the two
 *  results back in the inner components' types and synchronises, so that only stored-type bytes cross to the device and back;
 *  switches to the plans' device for the call.  The same dispatch and the same checks, on the host addresses. */
int fimex_amd_merge_apply_vector_typed_host(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                            const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                            const void* innerU, const fimex_amd_packing* innerUPacking, const void* innerV,
                                            const fimex_amd_packing* innerVPacking, const void* outerU, const fimex_amd_packing* outerUPacking,
                                            const void* outerV, const fimex_amd_packing* outerVPacking, size_t nz, void* outU, void* outV);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_MERGE_VECTOR_TYPED_HOST_H_ */
