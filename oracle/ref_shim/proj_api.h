/*
 * proj_api.h -- stand-in for PROJ.4's header of that name.  TEST INFRASTRUCTURE ONLY.
 *
 * The reference's src/interpolation.c includes "proj_api.h" and calls five pj_* functions.
 * This header declares them (PROJ.4's public signatures) so that the reference file compiles
 * unmodified; ref_shim.c defines them.  Everything else in interpolation.c is plain C whose
 * arithmetic does not depend on who declares these symbols.
 */
#ifndef ORACLE_REF_SHIM_PROJ_API_H_
#define ORACLE_REF_SHIM_PROJ_API_H_

#ifdef __cplusplus
extern "C" {
#endif

/* PROJ.4's values, to the digit */
#define RAD_TO_DEG 57.295779513082321
#define DEG_TO_RAD .017453292519943296

typedef void* projPJ;

extern int pj_errno;

projPJ pj_init_plus(const char* definition);
void pj_free(projPJ pj);
int pj_transform(projPJ src, projPJ dst, long point_count, int point_offset, double* x, double* y, double* z);
int pj_is_latlong(projPJ pj);
char* pj_strerrno(int err);

#ifdef __cplusplus
}
#endif
#endif
