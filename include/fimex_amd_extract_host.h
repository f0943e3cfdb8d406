/*
 * fimex_amd_extract_host.h -- the entries of the extraction block (8f n11) of fimex_amd.h that work on host buffers.
 * Same conventions as fimex_amd.h; a header of its own, as fimex_amd_derived_host.h and fimex_amd_time_quality_host.h are.
 */
#ifndef FIMEX_AMD_EXTRACT_HOST_H_
#define FIMEX_AMD_EXTRACT_HOST_H_

#include "fimex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/** fimex_amd_extract_apply_device on host buffers: switches to the plan's device, copies the whole source over, copies the result
 *  back and synchronises.  The same checks; outElements == 0 does nothing and accepts NULL pointers. */
int fimex_amd_extract_apply_host(const fimex_amd_extract_plan* plan, const void* in, int cdmType, void* out);

/**
 * CDMExtractor::reduceLatLonBoundingBox (src/CDMExtractor.cc:438-519) for one pair of 1-D axes: the mesh goes through
 * Projection::convertToLonLat (src/coordSys/Projection.cc:74-110; proj_input = getProj4String(), proj_lonlat = "+proj=latlong " +
 * getProj4EarthString(), axes multiplied by DEG_TO_RAD first when axesInDegree), and ix, iy of every point with
 * south <= lat <= north and its longitude in the box are kept; for west > east only lon > east && lon < west is outside.
 * xPositions[nx] and yPositions[ny] receive the ascending positions, *nX and *nY their counts: two fimex_amd_extract_dim.
 * A point whose transformation fails lies outside every box (divergence D10).  The box is checked as :442-447 do, before a device
 * is touched.  Host arrays throughout; the call synchronises.  nx == 0 or ny == 0 gives two empty lists.
 */
int fimex_amd_extract_bounding_box_host(const char* proj_input, const char* proj_lonlat, const double* xAxis, size_t nx,
                                        const double* yAxis, size_t ny, int axesInDegree, double south, double north, double west,
                                        double east, size_t* xPositions, size_t* nX, size_t* yPositions, size_t* nY);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_EXTRACT_HOST_H_ */
