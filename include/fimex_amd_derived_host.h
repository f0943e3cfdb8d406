/*
 * fimex_amd_derived_host.h -- the *_host forms of the entries of fimex_amd.h, section (8f n9): the same checks and the same work as
 * their *_device twins on host buffers.  Each call uploads its inputs, runs on a stream of its own, copies the result back and
 * returns when it is there; the inputs are left as they were.  The coefficient arrays of a level description are host arrays in
 * both forms; ps and field are host arrays here.  n == 0 (or nt == 0, an empty grid) does nothing and touches no pointer.
 * Plain C, like fimex_amd.h, which documents the arithmetic of every entry.
 */
#ifndef FIMEX_AMD_DERIVED_HOST_H_
#define FIMEX_AMD_DERIVED_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_convert_scaled_device on host arrays; out may be in itself when both types have the same size. */
int fimex_amd_convert_scaled_host(const void* in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType,
                                  double newFill, double newScale, double newOffset, void* out);

/** fimex_amd_theta_to_temperature_device on host arrays; T may be theta itself. */
int fimex_amd_theta_to_temperature_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* theta,
                                        float addOffset, float* T);

/** fimex_amd_specific_to_relative_humidity_device on host arrays. */
int fimex_amd_specific_to_relative_humidity_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* q,
                                                 const float* T, short* rh);

/** fimex_amd_accumulate_device on host arrays; prev: double[n], required when firstPos > 0. */
int fimex_amd_accumulate_host(const void* in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* prev, double* out);

/** fimex_amd_deaccumulate_device on host arrays; prev: n elements of cdmType, required when firstPos > 0. */
int fimex_amd_deaccumulate_host(const void* in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* prev, double* out);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_DERIVED_HOST_H_ */
