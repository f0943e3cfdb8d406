/*
 * fimex_amd_merge_typed_host.h -- the entries of the merge block of fimex_amd.h that work on variables in their stored types, on
 * host buffers.  Same conventions as fimex_amd.h; a header of its own, as the other late *_host entries have.  Only bytes of the
 * stored types cross to the device and back.
 */
#ifndef FIMEX_AMD_MERGE_TYPED_HOST_H_
#define FIMEX_AMD_MERGE_TYPED_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_border_smooth_typed_device on host arrays: copies both fields over in their stored types, copies the result back
 *  in the inner's type and synchronises.  The same checks. */
int fimex_amd_border_smooth_typed_host(const void* inner, const fimex_amd_packing* innerPacking, const void* outerOnInner,
                                       const fimex_amd_packing* outerPacking, void* out, size_t nx, size_t ny, size_t nz,
                                       size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined);
/** fimex_amd_overlay_typed_device on host arrays. */
int fimex_amd_overlay_typed_host(const void* top, const fimex_amd_packing* topPacking, const void* base,
                                 const fimex_amd_packing* basePacking, void* out, size_t n);
/** fimex_amd_merge_apply_typed_device on host arrays: switches to the plans' device for the call. */
int fimex_amd_merge_apply_typed_host(const fimex_amd_merge_plan* plan, const void* inner, const fimex_amd_packing* innerPacking,
                                     const void* outer, const fimex_amd_packing* outerPacking, size_t nz, void* out);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_MERGE_TYPED_HOST_H_ */
