/*
 * ref_shim.c -- what the reference's src/interpolation.c needs around it to become
 * oracle/_ref/libmifi_ref.so.  TEST INFRASTRUCTURE ONLY; our own text, nothing of the reference.
 *
 * Part 1: the pj_* symbols of proj_api.h.  No projection is computed here: pj_transform forwards
 *         to a hook the test installs (oracle/proj_oracle.py's transform), so the library pins the
 *         reference's own loops and arithmetic around the five calls, not the projections.
 * Part 2: batch drivers that loop over a position list in C, so that a test makes one ctypes call
 *         per case instead of one per point.
 */
#include "proj_api.h"

#include <stdlib.h>
#include <string.h>

#include "fimex/interpolation.h"

/* ------------------------------------------------------------------ part 1 */
int pj_errno = 0;

typedef int (*ref_shim_transform_fn)(const char* src, const char* dst, long n, double* x, double* y);
static ref_shim_transform_fn transform_hook = NULL;

void ref_shim_set_transform(ref_shim_transform_fn cb) { transform_hook = cb; }

projPJ pj_init_plus(const char* definition)
{
    if (definition == NULL) { pj_errno = -1; return NULL; }
    size_t len = strlen(definition);
    char* copy = (char*)malloc(len + 1);
    if (copy == NULL) { pj_errno = -1; return NULL; }
    memcpy(copy, definition, len + 1);
    return (projPJ)copy;
}

void pj_free(projPJ pj) { free(pj); }

/* value of "+proj=" in a definition: start and length, 0 when absent */
static size_t proj_name(const char* def, const char** start)
{
    const char* p = strstr(def, "proj=");
    /* "+proj=" of the top level comes first; "+o_proj=" also holds "proj=", so require '+' or start before it */
    while (p != NULL && p != def && p[-1] != '+' && p[-1] != ' ') p = strstr(p + 1, "proj=");
    if (p == NULL) return 0;
    p += 5;
    size_t n = 0;
    while (p[n] != '\0' && p[n] != ' ' && p[n] != '\t' && p[n] != '+') ++n;
    *start = p;
    return n;
}

/* PROJ.4: true for the four spellings of geographic coordinates only; ob_tran is not one of them */
int pj_is_latlong(projPJ pj)
{
    static const char* const names[] = {"latlong", "longlat", "latlon", "lonlat"};
    const char* s = NULL;
    if (pj == NULL) return 0;
    size_t n = proj_name((const char*)pj, &s);
    for (size_t i = 0; i < sizeof(names) / sizeof(names[0]); ++i)
        if (n == strlen(names[i]) && strncmp(s, names[i], n) == 0) return 1;
    return 0;
}

int pj_transform(projPJ src, projPJ dst, long point_count, int point_offset, double* x, double* y, double* z)
{
    (void)point_offset; (void)z;
    if (transform_hook == NULL || src == NULL || dst == NULL) { pj_errno = -1; return -1; }
    int rc = transform_hook((const char*)src, (const char*)dst, point_count, x, y);
    pj_errno = rc;
    return rc;
}

char* pj_strerrno(int err)
{
    (void)err;
    return (char*)"ref_shim: no transform hook set, or the hook failed";
}

/* ------------------------------------------------------------------ part 2 */
typedef int (*point_fn)(const float*, float*, const double, const double, const int, const int, const int);

/* method 0 / 1 / 2: mifi_get_values_f / _bilinear_f / _bicubic_f for every point i with skip[i] == 0.
 * out is [iz][n] (the layout CachedInterpolation::interpolateValues writes); cells of skipped points
 * are left as the caller filled them.  Returns MIFI_OK, or the first other return code met. */
int ref_shim_get_values_batch(int method, const float* infield, float* out, const double* px, const double* py,
                              const unsigned char* skip, long n, int ix, int iy, int iz)
{
    point_fn fn;
    switch (method) {
        case 0: fn = mifi_get_values_f; break;
        case 1: fn = mifi_get_values_bilinear_f; break;
        case 2: fn = mifi_get_values_bicubic_f; break;
        default: return MIFI_ERROR;
    }
    float* zValues = (float*)malloc((iz > 0 ? (size_t)iz : 1) * sizeof(float));
    if (zValues == NULL) return MIFI_ERROR;
    int ret = MIFI_OK;
    for (long i = 0; i < n; ++i) {
        if (skip != NULL && skip[i]) continue;
        int rc = fn(infield, zValues, px[i], py[i], ix, iy, iz);
        if (rc != MIFI_OK && ret == MIFI_OK) ret = rc;
        for (int z = 0; z < iz; ++z) out[(size_t)z * (size_t)n + (size_t)i] = zValues[z];
    }
    free(zValues);
    return ret;
}
