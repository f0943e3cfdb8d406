/*
 * fimex_amd_time_quality_host.h -- the *_host forms of the entries of fimex_amd.h, section (8f n10): the same checks and the same
 * work as their *_device twins on host buffers.  Each call uploads its inputs, runs on a stream of its own, copies the result back
 * and returns when it is there.  An empty call (n == 0, nNew == 0, nData == 0) does nothing and touches no data pointer.
 * Plain C, like fimex_amd.h, which documents the arithmetic of every entry.
 */
#ifndef FIMEX_AMD_TIME_QUALITY_HOST_H_
#define FIMEX_AMD_TIME_QUALITY_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_time_interpolate_device on host arrays: in [nOld][n] of cdmType, out float[nNew][n]; in is left as it was. */
int fimex_amd_time_interpolate_host(const void* in, int cdmType, size_t n, const double* oldTimes, size_t nOld, const double* newTimes,
                                    size_t nNew, float* out);

/** fimex_amd_quality_mask_device on host arrays, in place on data; status may be data itself (one type, nStatus == nData). */
int fimex_amd_quality_mask_host(void* data, int dataType, size_t nData, const void* status, int statusType, size_t nStatus, int mode,
                                const double* values, size_t nValues, double limit, double validMin, double validMax, double statusFill,
                                double fillValue);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_TIME_QUALITY_HOST_H_ */
