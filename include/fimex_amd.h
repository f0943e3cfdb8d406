/*
 * fimex_amd.h -- C ABI of the MI355X regridding engine (libfimex_amd.so).
 *
 * This is the drop-in boundary for the hot path of Fimex's CDMInterpolator
 * (L1 + L2 of SURVEY.md): what a maintainer binds from the reference's C++ in
 * place of the per-point mifi_* calls.  Every entry point cites the reference
 * interface it replaces (paths relative to the reference tree).  Plain pointers
 * and sizes only; no C++ or torch types.
 *
 * Conventions (same as the reference's C kernels, include/fimex/mifi_constants.h:259-261):
 *   return FIMEX_AMD_OK (1) or FIMEX_AMD_ERROR (-1); after an error
 *   fimex_amd_last_error() returns a message for the calling thread.
 *   Undefined values are IEEE NaN (mifi_constants.h:249-256).
 *   Fields are C arrays [nz][ny][nx], x fastest (include/fimex/interpolation.h:423-426).
 *
 * *_host entry points take host pointers (the reference's boost::shared_array
 * buffers), copy to the GPU, run the kernels and copy back; they are re-entrant
 * and may be called concurrently from several threads on one plan, as the
 * reference's writers do (src/NetCDF_CDMWriter.cc:749-753).
 * *_device entry points take device pointers plus a hipStream_t (passed as
 * void*; NULL = the default stream) and only enqueue work on that stream.
 *
 * There is no CPU fallback: every compute entry point fails with
 * FIMEX_AMD_ERROR when no gfx950 device is usable.
 */
#ifndef FIMEX_AMD_H_
#define FIMEX_AMD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIMEX_AMD_OK 1
#define FIMEX_AMD_ERROR -1

/* interpolation methods: values of enum mifi_interpol_method, include/fimex/mifi_constants.h:52-147 */
#define FIMEX_AMD_INTERPOL_NEAREST_NEIGHBOR 0
#define FIMEX_AMD_INTERPOL_BILINEAR 1
#define FIMEX_AMD_INTERPOL_BICUBIC 2
#define FIMEX_AMD_INTERPOL_COORD_NN 3
#define FIMEX_AMD_INTERPOL_COORD_NN_KD 4
#define FIMEX_AMD_INTERPOL_FORWARD_SUM 5
#define FIMEX_AMD_INTERPOL_FORWARD_MEAN 6
#define FIMEX_AMD_INTERPOL_FORWARD_MEDIAN 7
#define FIMEX_AMD_INTERPOL_FORWARD_MAX 8
#define FIMEX_AMD_INTERPOL_FORWARD_MIN 9
#define FIMEX_AMD_INTERPOL_FORWARD_UNDEF_SUM 10
#define FIMEX_AMD_INTERPOL_FORWARD_UNDEF_MEAN 11
#define FIMEX_AMD_INTERPOL_FORWARD_UNDEF_MEDIAN 12
#define FIMEX_AMD_INTERPOL_FORWARD_UNDEF_MAX 13
#define FIMEX_AMD_INTERPOL_FORWARD_UNDEF_MIN 14

/* axis types of mifi_points2position, include/fimex/mifi_constants.h:263-268 */
#define FIMEX_AMD_PROJ_AXIS 0
#define FIMEX_AMD_LONGITUDE 1
#define FIMEX_AMD_LATITUDE 2

/* ------------------------------------------------------------------ library */
/** Message of the last error raised on the calling thread ("" if none). */
const char* fimex_amd_last_error(void);
/** ABI version of this header (major*100 + minor). */
int fimex_amd_abi_version(void);
/** The *_host entry points stream caller buffers through pinned staging that is kept between calls (up to 4 idle sets of
 *  at most 384 MB pinned host memory and 384 MB - 1.1 GB of device memory each, allocated on first use; at most 8 in use at
 *  once, further concurrent callers wait).  This frees the idle ones. */
int fimex_amd_release_caches(void);
/** Number of usable gfx950 devices (0 when there is none; never an error). */
int fimex_amd_device_count(void);
/** Device the calling thread creates plans on (hipSetDevice). */
int fimex_amd_set_device(int ordinal);

/* ------------------------------------------------------------- regrid plans */
/**
 * Opaque, immutable regrid plan resident in HBM.  Replaces the state of
 * CachedInterpolation (include/fimex/CachedInterpolation.h:105-161: two
 * std::vector<double> + a function pointer) and of CachedForwardInterpolation
 * (src/CachedForwardInterpolation.h:37-59: two std::vector<int> + aggregator).
 */
typedef struct fimex_amd_regrid_plan fimex_amd_regrid_plan;

/**
 * Replaces the constructors CachedInterpolation::CachedInterpolation
 * (src/CachedInterpolation.cc:93-116) and
 * CachedForwardInterpolation::CachedForwardInterpolation
 * (src/CachedForwardInterpolation.cc:62-90) -- same arguments minus the
 * dimension names.
 *
 * funcType NEAREST_NEIGHBOR / BILINEAR / BICUBIC / COORD_NN / COORD_NN_KD:
 *   backward plan; pointsOnXAxis/pointsOnYAxis hold, per OUTPUT cell
 *   (nPoints == outX*outY), the fractional position in the input grid.
 * funcType FORWARD_*: forward plan; the arrays hold, per INPUT cell
 *   (nPoints == inX*inY), the fractional position in the output grid.
 * Any other funcType fails ("unknown interpolation function", as
 * CachedInterpolation.cc:114 / CachedForwardInterpolation.cc:88 throw).
 * The arrays are host memory and are not referenced after the call returns.
 */
int fimex_amd_regrid_plan_create(int funcType,
                                 const double* pointsOnXAxis, const double* pointsOnYAxis, size_t nPoints,
                                 size_t inX, size_t inY, size_t outX, size_t outY,
                                 fimex_amd_regrid_plan** plan);
/** Same, with the two position arrays already in device memory (plan build stays on the GPU). */
int fimex_amd_regrid_plan_create_device(int funcType,
                                        const double* d_pointsOnXAxis, const double* d_pointsOnYAxis, size_t nPoints,
                                        size_t inX, size_t inY, size_t outX, size_t outY,
                                        void* stream, fimex_amd_regrid_plan** plan);
/**
 * The same two constructors with the arithmetic of the bicubic kernel chosen per plan (ignored by every other method):
 *   FIMEX_AMD_BICUBIC_REFERENCE  the reference's operations in the reference's order -- products and row sums in double, four
 *                                accumulations into the float result (src/interpolation.c:1005-1019): bit-identical output;
 *   FIMEX_AMD_BICUBIC_FAST       weights rounded to float, float fused multiply-adds: differs from the reference by less than
 *                                1e-5 of the largest magnitude in the 4x4 stencil (typically 1e-7), and the launch is bound by
 *                                memory instead of by FP64 arithmetic.  NaN and out-of-domain behaviour are unchanged.
 */
#define FIMEX_AMD_BICUBIC_REFERENCE 0
#define FIMEX_AMD_BICUBIC_FAST 1
int fimex_amd_regrid_plan_create_opt(int funcType,
                                     const double* pointsOnXAxis, const double* pointsOnYAxis, size_t nPoints,
                                     size_t inX, size_t inY, size_t outX, size_t outY,
                                     int bicubicArithmetic, fimex_amd_regrid_plan** plan);
int fimex_amd_regrid_plan_create_device_opt(int funcType,
                                            const double* d_pointsOnXAxis, const double* d_pointsOnYAxis, size_t nPoints,
                                            size_t inX, size_t inY, size_t outX, size_t outY,
                                            int bicubicArithmetic, void* stream, fimex_amd_regrid_plan** plan);
int fimex_amd_regrid_plan_destroy(fimex_amd_regrid_plan* plan);

typedef struct fimex_amd_plan_info {
    int funcType;
    int device;                /* HIP ordinal the plan lives on */
    size_t inX, inY, outX, outY;
    size_t planBytes;          /* bytes of plan one apply launch reads (B_plan of DESIGN.md) */
    size_t undefinedCells;     /* backward: output cells that are NaN for every input; forward: empty buckets */
    size_t borderCells;        /* backward bilinear: cells on a border branch (interpolation.c:903-948) */
    size_t maxBucket;          /* forward: largest bucket (source cells per target) */
    size_t mappedSourceCells;  /* forward: source cells that fall inside the target grid */
    size_t stagedCells;        /* LDS-staged kernels (backward; forward plans with long buckets): source cells streamed per slice over all tiles (0: gather / lane kernels) */
    size_t tileW, tileH;       /* LDS-staged kernels: output cells per tile */
    size_t launchOrder;        /* LDS-staged float launches of 104 slices and more: 0 an XCD runs whole tiles, 1 an XCD runs one z chunk of every tile (set by fimex_amd_regrid_plan_tune_device; same results).  The newest field: callers of fimex_amd_regrid_plan_info built before it existed must be rebuilt, the library fills the whole struct */
} fimex_amd_plan_info;
int fimex_amd_regrid_plan_info(const fimex_amd_regrid_plan* plan, fimex_amd_plan_info* info);

/**
 * Replaces CachedInterpolationInterface::interpolateValues
 * (include/fimex/CachedInterpolation.h:67; src/CachedInterpolation.cc:118-147,
 * src/CachedForwardInterpolation.cc:92-131).
 * inData: host [size/(inX*inY)][inY][inX], not modified.
 * outData: host buffer the caller owns (the reference allocates it itself,
 * CachedInterpolation.cc:123); outCapacity in floats must be >= *newSize.
 * *newSize = outX*outY*(size/(inX*inY)), as CachedInterpolation.cc:120-122.
 * Pass outData == NULL to query *newSize only.
 */
int fimex_amd_regrid_apply_host(const fimex_amd_regrid_plan* plan,
                                const float* inData, size_t size,
                                float* outData, size_t outCapacity, size_t* newSize);
/** Device-resident form: d_in [nz][inY][inX] -> d_out [nz][outY][outX], enqueued on stream. */
int fimex_amd_regrid_apply_device(const fimex_amd_regrid_plan* plan,
                                  const float* d_in, size_t nz, float* d_out, void* stream);

/**
 * Optional, no counterpart in the reference: a bilinear plan (and a bicubic one with FIMEX_AMD_BICUBIC_FAST) holds its LDS-staged form in two workgroup shapes with identical
 * results, and which of them is faster depends on the device at hand and on the batch length.  This call regrids
 * the caller's nz slices a few times with each shape (d_out ends up holding the regridded slices), keeps the faster one for every
 * later apply of this plan and reports it in *chosenShape (0: the default shape, 1: the other; NULL allowed).  Plans without a
 * second shape and batches too short for the staged kernels return 0 at once.  Synchronises the stream; not to be called while
 * other threads apply the same plan.
 */
int fimex_amd_regrid_plan_tune_device(fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, float* d_out, void* stream,
                                      int* chosenShape);

/**
 * The same call also chooses between two launch orders of the LDS-staged float kernels, again with identical results: an XCD
 * (one of the chip's eight dies, each with its own L2) runs all z chunks of its tiles, the default, or one z chunk of every tile,
 * which needs 8 or 16 z chunks and so a batch of at least 104 slices.  The second order is timed on the winning shape and kept by
 * the same 1 % rule; fimex_amd_plan_info.launchOrder reports it.  This query answers for one batch length what
 * fimex_amd_regrid_apply_device would launch: *order = 1 whole tiles per XCD, 2 z chunks per XCD, 0 the chunk-major order of the
 * tuning build, -1 the batch does not run the LDS-staged float kernel of the second form.
 */
int fimex_amd_regrid_plan_launch_order(const fimex_amd_regrid_plan* plan, size_t nz, int* order);

/**
 * Cross-check, no counterpart in the reference: the same regrid through the per-lane gather kernels (one lane per output cell
 * reads its stencil straight from memory) whatever LDS-staged form the plan holds.  Backward plans only.  The result equals
 * fimex_amd_regrid_apply_device's bit for bit (FIMEX_AMD_BICUBIC_FAST plans: the reference's arithmetic, i.e. within the stated
 * 1e-5); bench.py and the tests use it to check EVERY slice of a long batch on the device.
 */
int fimex_amd_regrid_apply_gather_device(const fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, float* d_out, void* stream);

/* ------------------------------ source and output batches placed by the library */
/**
 * The reference allocates the result of every interpolateValues call itself (src/CachedInterpolation.cc:123) and receives its input
 * from the reader.  A caller that keeps its slices in device memory allocates the source batch [nz][inY][inX] and the output batch
 * [nz][outY][outX] once -- and which allocation they lie in moves the apply launch by several per cent (the source's
 * by 4-5 %, the output's by 1-3 %).  These two calls allocate the batches for the caller: `candidates` whole allocations are made and
 * held at once, the plan's apply launch is timed with each in its role (median of three launches), the fastest is kept and the others
 * are freed before the call returns.
 *   fimex_amd_regrid_source_batch_alloc_device  the buffer the caller's reader fills: every candidate is zero-filled and regridded
 *                                               into a scratch output; the kept one holds zeros.  Allocate this one first.
 *   fimex_amd_regrid_batch_alloc_device         the output batch: the caller's source batch d_in is regridded into every candidate
 *                                               (the batch holds the regridded slices of d_in afterwards only by accident).
 * candidates == 1: a plain allocation, nothing is timed (d_in may be NULL).  Fewer candidates are tried when device memory is short.
 * Both synchronise the stream.
 */
#define FIMEX_AMD_BATCH_MAX_POSITIONS 16
typedef struct fimex_amd_batch fimex_amd_batch;
typedef struct fimex_amd_batch_info {
    void* d_data;        /* the batch in device memory (plain hipMalloc memory) */
    size_t bytes;        /* of the batch */
    size_t bytesProbed;  /* device memory allocated while the candidates were tried */
    size_t bytesHeld;    /* device memory behind this batch after the call (== bytes) */
    size_t stepBytes;    /* 0 (candidates are separate allocations) */
    int positions;       /* candidates tried */
    int chosen;          /* the one that was kept */
    int trimmed;         /* 1: the other candidates were freed */
    float msAtPosition[FIMEX_AMD_BATCH_MAX_POSITIONS];  /* median time of the apply launch with each candidate */
    double probeSeconds; /* wall time of the whole call */
} fimex_amd_batch_info;
int fimex_amd_regrid_source_batch_alloc_device(const fimex_amd_regrid_plan* plan, size_t nz, int candidates, void* stream,
                                               fimex_amd_batch** batch);
int fimex_amd_regrid_batch_alloc_device(const fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, int candidates, void* stream,
                                        fimex_amd_batch** batch);
int fimex_amd_batch_get_info(const fimex_amd_batch* batch, fimex_amd_batch_info* info);
int fimex_amd_batch_free(fimex_amd_batch* batch);

/* ---------------------------------------------------------- vector rotation */
/**
 * Opaque rotation plan.  Replaces CachedVectorReprojection
 * (include/fimex/CachedVectorReprojection.h:33-63): built from the same
 * double[4*ox*oy] matrix (cos, sin, -sin, phi per cell, src/interpolation.c:429-432).
 * The matrix is copied; a compact (cos,sin) / phi form is kept in HBM.
 */
typedef struct fimex_amd_vector_plan fimex_amd_vector_plan;
int fimex_amd_vector_plan_create(const double* matrix, size_t ox, size_t oy, fimex_amd_vector_plan** plan);
int fimex_amd_vector_plan_destroy(fimex_amd_vector_plan* plan);
/** Replaces CachedVectorReprojection::reprojectValues (src/CachedVectorReprojection.cc:35-44) ->
 *  mifi_vector_reproject_values_by_matrix_f (src/interpolation.c:790-812); u, v rotated in place. */
int fimex_amd_vector_reproject_values_host(const fimex_amd_vector_plan* plan, float* u, float* v, size_t size);
int fimex_amd_vector_reproject_values_device(const fimex_amd_vector_plan* plan, float* d_u, float* d_v, size_t oz, void* stream);
/** Replaces CachedVectorReprojection::reprojectDirectionValues (src/CachedVectorReprojection.cc:46-55) ->
 *  mifi_vector_reproject_direction_by_matrix_f (src/interpolation.c:814-835); degrees, in place. */
int fimex_amd_vector_reproject_direction_host(const fimex_amd_vector_plan* plan, float* angles, size_t size);
int fimex_amd_vector_reproject_direction_device(const fimex_amd_vector_plan* plan, float* d_angles, size_t oz, void* stream);
/** CDMInterpolator::getDataSlice for an x/y vector pair (src/CDMInterpolator.cc:259-277):
 *  interpolateValues on both components, then CachedVectorReprojection::reprojectValues, in one call.
 *  d_u, d_v: [nz][inY][inX]; d_uOut, d_vOut: [nz][outY][outX]; none of the four may overlap another.
 *  The plan is a backward one, the vector plan has the plan's output grid and lives on the plan's device.
 *  *path (NULL allowed): 1 the fused kernel ran (nearest and bilinear plans with an LDS-staged form, batches of four pairs
 *  and more), 0 the three existing launches (regrid_apply on u and on v, vector_reproject_values); the same bits either way.
 *  The *_host form is declared in fimex_amd_vector_regrid_host.h. */
int fimex_amd_regrid_apply_vector_device(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec,
                                         const float* d_u, const float* d_v, size_t nz,
                                         float* d_uOut, float* d_vOut, void* stream, int* path);
/** The same on a pair in its stored types (src/CDMInterpolator.cc:251-285 without pre- and post-processes, both components at
 *  once): each component is read as data2InterpolationArray reads it (Data::asFloat, then mifi_bad2nanf with its own fill
 *  value), both are regridded and rotated, and each comes back as interpolationArray2Data(own type, own fill value).
 *  d_u, d_uOut hold elements of uType, d_v, d_vOut of vType (fimex_amd_datatype, all ten numeric types; the two may differ);
 *  layouts, plans and refusals as above, with buffer sizes counted in each buffer's own element size.
 *  *path (NULL allowed): 2 one kernel on the stored type, no float copy of a slice (both components SHORT or both USHORT,
 *  nearest and bilinear plans whose source slice is a multiple of 4 bytes and that hold a staged form for 2-byte elements,
 *  4-byte aligned d_u and d_v, four pairs and more); 1 or 0 the chain of five launches around the float pair entry -- to
 *  float twice, fimex_amd_regrid_apply_vector_device (whose path this is), back twice -- on temporaries of
 *  2*4*nz*(inX*inY + outX*outY) bytes, released after a stream synchronisation.  The same bytes either way.
 *  The *_host form is declared in fimex_amd_vector_regrid_typed_host.h. */
int fimex_amd_regrid_apply_vector_typed_device(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec,
                                               const void* d_u, int uType, double uBad,
                                               const void* d_v, int vType, double vBad, size_t nz,
                                               void* d_uOut, void* d_vOut, void* stream, int* path);

/* ------------------------------------------------------ 2-D fill processes */
/*
 * Batch forms of the InterpolatorProcess2d implementations
 * (include/fimex/CDMInterpolator.h:49-88) as driven by processArray_
 * (src/CDMInterpolator.cc:136-159): every [ny][nx] slice of field[nz][ny][nx] is
 * filled in place, independently.  nChanged: NULL or size_t[nz] receiving the
 * per-slice count of undefined cells the reference returns through *nChanged.
 */
/** mifi_fill2d_f, include/fimex/interpolation.h:483, src/interpolation.c:1246-1376 */
int fimex_amd_fill2d_host(size_t nx, size_t ny, size_t nz, float* field,
                          float relaxCrit, float corrEff, size_t maxLoop, size_t* nChanged);
int fimex_amd_fill2d_device(size_t nx, size_t ny, size_t nz, float* d_field,
                            float relaxCrit, float corrEff, size_t maxLoop, size_t* nChanged, void* stream);
/** mifi_creepfill2d_f, include/fimex/interpolation.h:505, src/interpolation.c:1495-1519 */
int fimex_amd_creepfill2d_host(size_t nx, size_t ny, size_t nz, float* field,
                               unsigned short repeat, char setWeight, size_t* nChanged);
int fimex_amd_creepfill2d_device(size_t nx, size_t ny, size_t nz, float* d_field,
                                 unsigned short repeat, char setWeight, size_t* nChanged, void* stream);
/** mifi_creepfillval2d_f, include/fimex/interpolation.h:528, src/interpolation.c:1521-1537 */
int fimex_amd_creepfillval2d_host(size_t nx, size_t ny, size_t nz, float* field, float defaultVal,
                                  unsigned short repeat, char setWeight, size_t* nChanged);
int fimex_amd_creepfillval2d_device(size_t nx, size_t ny, size_t nz, float* d_field, float defaultVal,
                                    unsigned short repeat, char setWeight, size_t* nChanged, void* stream);

/* ------------------------------------------- the whole per-slice sequence */
/** One registered 2-D process: the parameters of InterpolatorFill2d / InterpolatorCreepFill2d /
 *  InterpolatorCreepFillVal2d (include/fimex/CDMInterpolator.h:55-88). */
#define FIMEX_AMD_PROCESS_FILL2D 1
#define FIMEX_AMD_PROCESS_CREEPFILL2D 2
#define FIMEX_AMD_PROCESS_CREEPFILLVAL2D 3
typedef struct fimex_amd_process2d {
    int kind;               /* FIMEX_AMD_PROCESS_* */
    float relaxCrit;        /* fill2d */
    float corrEff;          /* fill2d */
    size_t maxLoop;         /* fill2d */
    unsigned short repeat;  /* creepfill */
    char setWeight;         /* creepfill */
    float defaultVal;       /* creepfillval2d */
} fimex_amd_process2d;

/**
 * Replaces the body of CDMInterpolator::getDataSlice between reading the input and converting the output
 * (src/CDMInterpolator.cc:255-285) with the data staying in HBM between the steps:
 *   fill value -> NaN (:115-119), pre-processes per z slice (:256, :136-159), interpolateValues (:259),
 *   for an x/y vector component: the same on the counterpart, then reprojectValues (:261-283),
 *   post-processes (:284), NaN -> fill value (:285, without the type conversion, which stays with Data).
 * inData / counterpart: host [size/(inX*inY)][inY][inX]; badValue*: the variables' fill values (NaN = none).
 * counterpart == NULL or vec == NULL: scalar variable.  isXComponent != 0: inData is the x component (u) and
 * counterpart the y component (v); otherwise the other way round; outData receives the requested component.
 * pre / post: the registered processes in order (may be NULL when the count is 0).
 * outData == NULL queries *newSize only.
 */
int fimex_amd_regrid_slice_host(const fimex_amd_regrid_plan* plan, const float* inData, size_t size, float badValue,
                                const fimex_amd_process2d* pre, size_t nPre,
                                const float* counterpart, float badValueCounterpart,
                                const fimex_amd_vector_plan* vec, int isXComponent,
                                const fimex_amd_process2d* post, size_t nPost,
                                float* outData, size_t outCapacity, size_t* newSize);

/* ------------------------------------------------- edges of the path (a13) */
/** mifi_bad2nanf / mifi_nanf2bad, src/interpolation.c:1775-1793, on n device floats in place. */
int fimex_amd_bad2nan_device(float* d_data, size_t n, float badVal, void* stream);
int fimex_amd_nan2bad_device(float* d_data, size_t n, float badVal, void* stream);

/** CDMProcessor's direction rotation of packed angles (src/CDMProcessor.cc:621-636): scale * a + offset, rotate
 *  (a9), (a - offset) / scale, in one pass; angles [oz][oy][ox] in place. */
int fimex_amd_vector_reproject_direction_scaled_host(const fimex_amd_vector_plan* plan, float* angles, size_t size, double scale, double offset);
int fimex_amd_vector_reproject_direction_scaled_device(const fimex_amd_vector_plan* plan, float* d_angles, size_t oz, double scale,
                                                       double offset, void* stream);

/* ------------------------------------------------ typed slices */
/** CDMDataType, include/fimex/CDMDataType.h:35-49 (same values). */
typedef enum fimex_amd_datatype {
    FIMEX_AMD_CDM_NAT = 0, FIMEX_AMD_CDM_CHAR, FIMEX_AMD_CDM_SHORT, FIMEX_AMD_CDM_INT, FIMEX_AMD_CDM_FLOAT,
    FIMEX_AMD_CDM_DOUBLE, FIMEX_AMD_CDM_STRING, FIMEX_AMD_CDM_UCHAR, FIMEX_AMD_CDM_USHORT, FIMEX_AMD_CDM_UINT,
    FIMEX_AMD_CDM_INT64, FIMEX_AMD_CDM_UINT64
} fimex_amd_datatype;
/** data2InterpolationArray, src/CDMInterpolator.cc:115-119: n device elements of cdmType -> float (Data::asFloat())
 *  with the variable's fill value as NaN (mifi_bad2nanf), in one pass. */
int fimex_amd_data2interpolation_device(const void* d_in, int cdmType, size_t n, double badValue, float* d_out, void* stream);
/** interpolationArray2Data, src/CDMInterpolator.cc:121-124: float -> cdmType as
 *  DataImpl<float>::convertDataType(MIFI_UNDEFINED_F, 1, 0, cdmType, badValue, 1, 0) does (NaN -> fill value,
 *  integers rounded through MetNoFimex::round), in one pass. */
int fimex_amd_interpolation2data_device(const float* d_in, size_t n, int cdmType, double badValue, void* d_out, void* stream);
/** interpolateValues on device-resident slices of a variable's stored type: d_in [nz][inY][inX] elements of cdmType ->
 *  d_out [nz][outY][outX] elements of the same type, i.e. data2InterpolationArray, the regrid and interpolationArray2Data
 *  of src/CDMInterpolator.cc:251-285 without pre/post-processes.  For backward plans on 1-, 2-byte and 32-bit integer
 *  types this is ONE kernel that reads and writes the stored type (no float copy of the slices exists); other
 *  combinations run the three passes on temporaries. */
int fimex_amd_regrid_apply_typed_device(const fimex_amd_regrid_plan* plan, const void* d_in, int cdmType, size_t nz,
                                        double badValue, void* d_out, void* stream);
/**
 * A LIST of variables on one plan in one call: what nvar calls of fimex_amd_regrid_apply_device (of
 * fimex_amd_regrid_apply_typed_device with badValue[i]) compute, byte for byte, for every plan kind and every numeric type those
 * entries accept.  The reference calls CDMInterpolator::getDataSlice once per variable and time step
 * (src/CDMInterpolator.cc:251-259); a writer hands one time step's variables of a grid over at once instead, each still an
 * allocation of its own -- mostly surface fields of one slice, which alone are too short for the LDS-staged kernels.
 *
 * d_in, nz, badValue and d_out are HOST arrays of nvar entries, d_in[i] a device array [nz[i]][inY][inX] and d_out[i]
 * [nz[i]][outY][outX]; the call only enqueues on `stream` and has read the four arrays when it returns.  nvar == 0 and
 * nz[i] == 0 are successful no-ops that need no device (d_in[i], d_out[i] may then be NULL).  An input may appear more than once;
 * outputs must not overlap each other or any input: such a call is refused and nothing is launched.  Pointers are aligned to the
 * element size and nothing more.
 *
 * *path (NULL allowed): 1 = the slices ran through the list kernels of the second LDS-staged form, in launches of at most
 * FIMEX_AMD_REGRID_MULTI_MAX_VARS variables; 0 = the per-variable calls ran inside the entry.  The list kernels run when the
 * SUM of nz[] is a batch of that form -- nearest, bilinear and FIMEX_AMD_BICUBIC_FAST plans that hold it, at least 4 slices in
 * all -- and, typed entry, the type has 1 or 2 bytes and every d_in[i] is 4-byte aligned.  Bicubic plans in the reference's
 * arithmetic, forward plans, plans without a staged form, 4- and 8-byte types and shorter lists take path 0.
 */
#define FIMEX_AMD_REGRID_MULTI_MAX_VARS 64   /* variables one list launch takes; more run in several launches */
int fimex_amd_regrid_apply_multi_device(const fimex_amd_regrid_plan* plan, size_t nvar, const float* const* d_in, const size_t* nz,
                                        float* const* d_out, void* stream, int* path);
int fimex_amd_regrid_apply_multi_typed_device(const fimex_amd_regrid_plan* plan, size_t nvar, const void* const* d_in, int cdmType,
                                              const size_t* nz, const double* badValue, void* const* d_out, void* stream, int* path);
/* The *_host forms are declared in fimex_amd_regrid_multi_host.h. */
/** The same two conversions on host buffers (copied to the GPU and back), for callers that run their own 2-D processes
 *  on the float array in between. */
int fimex_amd_data2interpolation_host(const void* in, int cdmType, size_t n, double badValue, float* out);
int fimex_amd_interpolation2data_host(const float* in, size_t n, int cdmType, double badValue, void* out);
/** fimex_amd_regrid_slice_host on the variable's stored type: everything CDMInterpolator::getDataSlice
 *  (src/CDMInterpolator.cc:251-285) does with a slice, including both conversions; only `size` elements of dataType
 *  cross PCIe in, *newSize elements of dataType come back (half the bytes for packed shorts).  size and outCapacity
 *  count elements.  The counterpart of a vector variable may be stored in another type. */
int fimex_amd_regrid_slice_typed_host(const fimex_amd_regrid_plan* plan, const void* inData, int dataType, size_t size, double badValue,
                                      const fimex_amd_process2d* pre, size_t nPre,
                                      const void* counterpart, int counterpartType, double badValueCounterpart,
                                      const fimex_amd_vector_plan* vec, int isXComponent,
                                      const fimex_amd_process2d* post, size_t nPost,
                                      void* outData, size_t outCapacity, size_t* newSize);

/** CDMProcessor::getDataSlice's vector rotation on stored types (src/CDMProcessor.cc:590-618): both components become
 *  float/NaN (data2InterpolationArray), are rotated in place (a8), and the requested one (returnX != 0: x) comes back in
 *  outType with outFill as interpolationArray2Data does.  size elements per component, [size/(ox*oy)][oy][ox]. */
int fimex_amd_rotate_vector_typed_host(const fimex_amd_vector_plan* plan, const void* xData, int xType, double xFill,
                                       const void* yData, int yType, double yFill, size_t size, int returnX,
                                       int outType, double outFill, void* outData);

/* ------------------------------------------------------- plan build helpers */
/** mifi_points2position, include/fimex/interpolation.h:415, src/interpolation.c:148-217:
 *  n device doubles (radians or metres) -> fractional axis indices, in place. axis: host, num entries. */
int fimex_amd_points2position_device(double* d_points, size_t n, const double* axis, int num, int axis_type, void* stream);
/** Same on n host doubles (copied to the GPU and back). */
int fimex_amd_points2position_host(double* points, size_t n, const double* axis, int num, int axis_type);

/* ------------------------------------------ 1-D blends between two fields (8f n4) */
/** mifi_get_values_{nearest, linear, linear_weak_extrapol, linear_no_extrapol, linear_const_extrapol, log, log_log}_f
 *  (include/fimex/interpolation.h, src/interpolation.c:1030-1156): outfield = blend of infieldA (at coordinate a) and
 *  infieldB (at b) at coordinate x, n values, as the time and vertical interpolators call them.  out may alias A or B.
 *  Returns FIMEX_AMD_ERROR where the reference returns MIFI_ERROR (non-positive a, b or x for the log blends). */
typedef enum fimex_amd_blend1d {
    FIMEX_AMD_1D_NEAREST = 0, FIMEX_AMD_1D_LINEAR, FIMEX_AMD_1D_LINEAR_WEAK_EXTRAPOL, FIMEX_AMD_1D_LINEAR_NO_EXTRAPOL,
    FIMEX_AMD_1D_LINEAR_CONST_EXTRAPOL, FIMEX_AMD_1D_LOG, FIMEX_AMD_1D_LOG_LOG
} fimex_amd_blend1d;
int fimex_amd_get_values_1d_f_device(int kind, const float* d_infieldA, const float* d_infieldB, float* d_outfield, size_t n,
                                     double a, double b, double x, void* stream);
int fimex_amd_get_values_1d_f_host(int kind, const float* infieldA, const float* infieldB, float* outfield, size_t n,
                                   double a, double b, double x);
/** mifi_get_values_linear_d, src/interpolation.c:1065-1083. */
int fimex_amd_get_values_linear_d_device(const double* d_infieldA, const double* d_infieldB, double* d_outfield, size_t n,
                                         double a, double b, double x, void* stream);

/* ------------------------------------------------ vertical interpolation (8f n5) */
/** Values of enum mifi_vertical_interpol_method, include/fimex/mifi_constants.h:202-231. */
#define FIMEX_AMD_VINT_METHOD_LIN 0
#define FIMEX_AMD_VINT_METHOD_LOG 1
#define FIMEX_AMD_VINT_METHOD_LOGLOG 2
#define FIMEX_AMD_VINT_METHOD_NN 3
#define FIMEX_AMD_VINT_METHOD_LIN_WEAK_EXTRA 4
#define FIMEX_AMD_VINT_METHOD_LIN_NO_EXTRA 5
#define FIMEX_AMD_VINT_METHOD_LIN_CONST_EXTRA 6

/** How the levels of a column are given: what the reference's VerticalConverter would put into verticalData4D. */
#define FIMEX_AMD_VLEVEL_FIELD 0            /* explicit f32 field [nt][nz][ny][nx] */
#define FIMEX_AMD_VLEVEL_AXIS 1             /* axis[nz], the same in every column (pressure / height axis, IdentityConverter) */
#define FIMEX_AMD_VLEVEL_SIGMA 2            /* ptop + sigma[k] * (ps - ptop), src/vertical_coordinate_transformations.c:37-44 */
#define FIMEX_AMD_VLEVEL_HYBRID_SIGMA 3     /* a[k] * p0 + b[k] * ps, :57-63 */
#define FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP 4  /* ap[k] + b[k] * ps, :65-71 */

/**
 * The levels of every column of a [nt][nz][ny][nx] variable.  Formula kinds are evaluated in double in the reference's
 * operation order and rounded to float (Data::asFloat()); nothing 3-D exists in memory for them.
 * axis, sigma, a, ap, b: HOST arrays of nz doubles in the *_device and the *_host entry points alike; they are copied by
 * the call.  ps ([nt][ny][nx], already in the unit of the coefficients) and field follow the entry point: device pointers
 * for *_device, host pointers for *_host.  Members a kind does not use are ignored.
 */
typedef struct fimex_amd_vertical_levels {
    int kind;             /* FIMEX_AMD_VLEVEL_* */
    size_t nz;
    const double* axis;   /* AXIS */
    const double* sigma;  /* SIGMA */
    const double* a;      /* HYBRID_SIGMA */
    const double* ap;     /* HYBRID_SIGMA_AP */
    const double* b;      /* HYBRID_SIGMA, HYBRID_SIGMA_AP */
    double p0;            /* HYBRID_SIGMA */
    double ptop;          /* SIGMA */
    const float* ps;      /* SIGMA, HYBRID_SIGMA, HYBRID_SIGMA_AP */
    const float* field;   /* FIELD */
} fimex_amd_vertical_levels;

/**
 * Replaces the loop of CDMVerticalInterpolator::getLevelDataSlice (src/CDMVerticalInterpolator.cc:441-504) for a batch of nt
 * unlimited-dimension positions: d_in [nt][inLevels->nz][ny][nx] -> d_out [nt][nzo][ny][nx].  Per column and output level:
 * the target level x is level1[k] (outLevels == NULL: fixed levels, host double[nzo]) or the level outLevels describes
 * (interpolateByTemplateVariable; nzo must equal outLevels->nz, level1 is ignored); x outside [validMin, validMax] of the
 * column (double[ny][nx] each, NULL: no bound) gives NaN (:454-471); the bracketing input levels are those of
 * find_closest_neighbor_distinct_elements (include/fimex/Utils.h:204-290) run over the column in index order; the two data
 * values are blended by mifi_get_values_*_f with n = 1 (src/interpolation.c:1030-1156); the result is clamped to
 * [clampMin, clampMax] (NaN: no bound; :494-504).
 * One divergence: where the log blends return MIFI_ERROR (a non-positive level) the reference leaves the output element
 * uninitialised; NaN is written here.
 * Only enqueues work on the stream and never synchronises it.  d_out must not overlap d_in.
 */
int fimex_amd_vertical_interpolate_device(int method, size_t nx, size_t ny, size_t nt, const float* d_in,
                                          const fimex_amd_vertical_levels* inLevels, const fimex_amd_vertical_levels* outLevels,
                                          const double* level1, size_t nzo, const double* d_validMin, const double* d_validMax,
                                          float clampMin, float clampMax, float* d_out, void* stream);
/** The same on host buffers (in, inLevels->ps / ->field, outLevels->ps / ->field, validMin, validMax, out). */
int fimex_amd_vertical_interpolate_host(int method, size_t nx, size_t ny, size_t nt, const float* in,
                                        const fimex_amd_vertical_levels* inLevels, const fimex_amd_vertical_levels* outLevels,
                                        const double* level1, size_t nzo, const double* validMin, const double* validMax,
                                        float clampMin, float clampMax, float* out);
/** What verticalData4D returns for a level description: the f32 field [nt][levels->nz][ny][nx]. */
int fimex_amd_vertical_levels_device(const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, float* d_out, void* stream);
int fimex_amd_vertical_levels_host(const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, float* out);

/* ------------------------------- vertical interpolation plans (8f n5b) */
/* The search of fimex_amd_vertical_interpolate_* depends on the input levels, the target levels, the validity range and the method,
 * never on the variable.  A plan holds its result per (unlimited-dimension position, output level, column): the pair of input
 * levels and the blend factor with the method folded in, 8 bytes per output cell.  The apply gathers two values per cell, blends,
 * clamps and stores, on the variable's stored type and for several variables in one call.  The reference has no such object: the
 * arithmetic is getLevelDataSlice's, the split is this library's. */

/** Opaque, immutable vertical interpolation plan, resident in HBM. */
typedef struct fimex_amd_vertical_plan fimex_amd_vertical_plan;

typedef struct fimex_amd_vertical_info {
    size_t nx, ny, nt;
    size_t nzi, nzo;
    int method;         /* FIMEX_AMD_VINT_METHOD_* */
    size_t entryBytes;  /* bytes of the entries on the device */
} fimex_amd_vertical_info;

/**
 * Runs the search of fimex_amd_vertical_interpolate_device for every output cell and keeps its result; every argument means what
 * it means there.  Allocates the entries on the calling thread's device, enqueues the build on `stream` and returns.  ps, field,
 * d_validMin and d_validMax are read by the build only; level1 and the coefficient arrays are free on return.  The plan may be
 * applied on the same stream at once, and on another stream once the caller has ordered that stream behind the build.
 * Refused, before any device is initialised: an unknown method or level kind, NULL where a kind needs an array, fixed levels
 * without level1, nzi == 0, nzo == 0, nzi > 65535 (an entry holds a level index in 16 bits), nt > 65535.
 * Lifetime, as for the other plan objects: the plan belongs to the device it was created on and to the library that made it;
 * it is immutable, so any number of threads and streams may apply it at once; destroy it only after every apply that was
 * enqueued with it has finished, and on no stream's behalf does the library wait for that.
 */
int fimex_amd_vertical_plan_create_device(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                                          const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo,
                                          const double* d_validMin, const double* d_validMax, void* stream,
                                          fimex_amd_vertical_plan** plan);
int fimex_amd_vertical_plan_destroy(fimex_amd_vertical_plan* plan);
int fimex_amd_vertical_plan_info(const fimex_amd_vertical_plan* plan, fimex_amd_vertical_info* info);
/**
 * getLevelDataSlice for nvar >= 1 variables that share the plan, on their stored type cdmType (one of the ten numeric
 * fimex_amd_datatype values): d_in[i] [nt][nzi][ny][nx] -> d_out[i] [nt][nzo][ny][nx] of the same type.  d_in, badValue, clampMin,
 * clampMax and d_out are HOST arrays of length nvar; d_in[] and d_out[] hold device pointers.  Per output cell: an undefined entry
 * gives NaN; otherwise A and B are the two data values as data2InterpolationArray reads them (static_cast to float, badValue[i]
 * as NaN; a NaN badValue changes nothing) and v = f == 0 ? A : f == 1 ? B : A + f * (B - A); v is clamped to
 * [clampMin[i], clampMax[i]] (NaN: no bound) and stored as interpolationArray2Data stores it (NaN as badValue[i], integers
 * rounded).  This is fimex_amd_data2interpolation_device, fimex_amd_vertical_interpolate_device and
 * fimex_amd_interpolation2data_device in one pass, byte for byte, with no float copy of the variable.  One case apart: cdmType
 * FLOAT with a NaN badValue is an interpolation array as fimex_amd_vertical_interpolate_device takes it; it is read and stored
 * unchanged and the result is that entry's bit for bit (the three calls would turn a -0.0 into +0.0).
 * The library groups the variables into launches of its choice; a launch reads the entries once for its variables.  Outputs must
 * not overlap each other, an input or the plan.  Pointers must be aligned to the element size, and nothing more.  Only enqueues
 * on `stream`; must run on the plan's device.
 */
int fimex_amd_vertical_plan_apply_device(const fimex_amd_vertical_plan* plan, size_t nvar, const void* const* d_in, int cdmType,
                                         const double* badValue, const float* clampMin, const float* clampMax, void* const* d_out,
                                         void* stream);
/* The *_host forms of create and apply, and the entries read back to the host, are declared in fimex_amd_vertical_plan_host.h. */

/* ------------------------ vertical level converters: altitude, height, depth (8f n6) */
/* What the reference's VerticalConverter chain (src/coordSys/verticalTransform/) puts into verticalData4D for the vertical
 * types MIFI_VINT_ALTITUDE, MIFI_VINT_HEIGHT and MIFI_VINT_DEPTH: an f32 field [nt][nz][ny][nx], which
 * fimex_amd_vertical_interpolate_* take as FIMEX_AMD_VLEVEL_FIELD.  Whole columns only.  The *_device entries only enqueue
 * work on the stream and never synchronise it; the *_host entries take host buffers for everything.  The coefficient arrays
 * of a level description, s and C are host arrays in both.  The output must not overlap any input. */

/** Which end of the vertical axis is next to the surface (surfaceFirst). */
#define FIMEX_AMD_VORDER_AUTO (-1)  /* decided as the reference does, see below */
#define FIMEX_AMD_VORDER_SURFACE_LAST 0
#define FIMEX_AMD_VORDER_SURFACE_FIRST 1

/**
 * PressureIntegrationToAltitudeConverter::getDataSlice (PressureIntegrationToAltitudeConverter.cc:85-210): the altitude of
 * every level by the hypsometric equation, integrated from the surface upward.  Per column: a = (double)sgp / 9.80665,
 * p_low = sap; per level, p_high = the level's pressure as float, Tv = T or mifi_virtual_temperature(q, T) (q != NULL),
 * a += (double)mifi_barometric_layer_thickness(p_low, p_high, Tv), p_low = p_high
 * (src/vertical_coordinate_transformations.c:108-111, :154-157).  A NaN makes the column NaN from that level upward.
 * pressure: the levels' pressure in the unit of surfacePressure (hPa in the reference); airTemperature and specificHumidity
 * [nt][nz][ny][nx]; surfacePressure and surfaceGeopotential (m^2/s^2) [nt][ny][nx].
 * surfaceFirst: 1 when level index 0 is next to the surface, 0 when the last index is, FIMEX_AMD_VORDER_AUTO to decide as the
 * reference does (:105-122): index 0 is at the surface when the first level's pressure is greater than the last level's (both
 * as float) in column x = 0, y = 0 of the batch's FIRST time step.  The reference looks at the file's first time step: a
 * caller whose batch does not start there passes 0 or 1 to match it.
 * topo == NULL: the result is (float)a.  Otherwise AltitudeHeightConverter::getDataSlice (AltitudeHeightConverter.cc:87-105)
 * follows on the unrounded a: (float)(a + topoFactor * topo), topo double[ny][nx], topoFactor -1 (altitude to height) or +1,
 * divided by 9.80665 when topo is a geopotential (:62-77).
 */
int fimex_amd_vertical_altitude_integrate_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                                 const float* d_airTemperature, const float* d_specificHumidity,
                                                 const float* d_surfacePressure, const float* d_surfaceGeopotential, int surfaceFirst,
                                                 const double* d_topo, double topoFactor, float* d_out, void* stream);
int fimex_amd_vertical_altitude_integrate_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                               const float* airTemperature, const float* specificHumidity,
                                               const float* surfacePressure, const float* surfaceGeopotential, int surfaceFirst,
                                               const double* topo, double topoFactor, float* out);

/**
 * PressureToStandardAltitudeConverter::getDataSlice (:33-41): (-BAROMETRIC_FACTOR * 288.15) * log(p / 1013.25) in double
 * (mifi_barometric_standard_altitude, src/vertical_coordinate_transformations.c:94-106), p in hPa.  The converter reads its
 * inner converter's DOUBLE data: a formula kind enters unrounded, a FIELD as its floats promoted, an AXIS as its doubles.
 * topo != NULL: (float)(altitude + topoFactor * topo) as above, otherwise (float)altitude.
 */
int fimex_amd_vertical_standard_altitude_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                                const double* d_topo, double topoFactor, float* d_out, void* stream);
int fimex_amd_vertical_standard_altitude_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                              const double* topo, double topoFactor, float* out);

/**
 * AltitudeStandardToPressureConverter::getDataSlice (:33-41): 1013.25 * exp((-1 / (BAROMETRIC_FACTOR * 288.15)) * h) in double
 * (mifi_barometric_standard_pressure, :79-91), hPa.  altitude: the levels in m, read as doubles as above.  topo != NULL: the
 * levels are heights and an AltitudeHeightConverter stands in front, h = level + topoFactor * topo (topoFactor +1, or
 * 1 / 9.80665 for a geopotential).
 */
int fimex_amd_vertical_standard_pressure_device(const fimex_amd_vertical_levels* altitude, size_t nx, size_t ny, size_t nt,
                                                const double* d_topo, double topoFactor, float* d_out, void* stream);
int fimex_amd_vertical_standard_pressure_host(const fimex_amd_vertical_levels* altitude, size_t nx, size_t ny, size_t nt,
                                              const double* topo, double topoFactor, float* out);

/**
 * OceanSCoordinateGToDepthConverter::getDataSlice (:66-107): depth, positive down, of ocean_s_coordinate_g1 / _g2 levels:
 * (float)(-z) with z of mifi_ocean_s_g1_z (generation 1) or mifi_ocean_s_g2_z (generation 2)
 * (src/vertical_coordinate_transformations.c:159-176).  s, C: host double[nz]; depth double[ny][nx]; eta double[nt][ny][nx] or
 * NULL for 0.  No transcendental is involved: the result is the reference's bit for bit.
 */
int fimex_amd_vertical_ocean_depth_device(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C,
                                          double depth_c, const double* d_depth, const double* d_eta, float* d_out, void* stream);
int fimex_amd_vertical_ocean_depth_host(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C,
                                        double depth_c, const double* depth, const double* eta, float* out);

/* ------------------------------------ vertical velocity on model levels (8f n7) */
/* What CDMProcessor::addVerticalVelocity (src/CDMProcessor.cc:158-318, :515-530) computes per time step, and the omega2vwind
 * conversion of CDMPressureConversions.  Layouts as above: x fastest, [nt][nz][ny][nx].  The *_device entries only enqueue work
 * on the stream and never synchronise it; the *_host entries take host buffers for everything.  ap and b are host double[nz] in
 * both. */

/**
 * mifi_griddistance (src/interpolation.c:1539-1595): lon, lat double[ny][nx] in degrees -> gridDistX, gridDistY float[ny][nx] in
 * m, the great-circle distance (float)(6371000 * acos(sin(la0) * sin(la1) + cos(la0) * cos(la1) * cos(lo1 - lo0))) of cell
 * p = i + nx * j to its right neighbour p + 1 (X) and to the next row's cell p + nx (Y), every angle multiplied by DEG_TO_RAD
 * = .017453292519943296 first, all in double.  The last column repeats the column before it.  The last row is filled as the
 * reference fills it, from i = 0 upward with g[p] = g[p - ny] (not p - nx): for i >= ny the source lies in the last row itself
 * and holds what was written there a moment earlier, so the value of cell i is that of cell i mod ny of the last row.
 * nx == 1 or ny == 1: the distance to the next point along the line in both outputs, the last point repeating the one before.
 * nx * ny == 1: zeros are written and -1 is returned, as the reference does.  The outputs must not overlap each other or an
 * input.  The device's sin, cos and acos are not the host's: a result is within 2^-23 * |d| + 6371000 * 2^-49 / sin(d / 6371000)
 * of the reference's.
 */
int fimex_amd_griddistance_device(size_t nx, size_t ny, const double* d_lon, const double* d_lat, float* d_gridDistX, float* d_gridDistY,
                                  void* stream);
int fimex_amd_griddistance_host(size_t nx, size_t ny, const double* lon, const double* lat, float* gridDistX, float* gridDistY);

/**
 * mifi_compute_vertical_velocity (src/interpolation.c:1597-1773) for nt time steps: upward_air_velocity_ml in m/s on hybrid
 * levels, index 0 at the top.  dx, dy: the grid spacing of the projection axes in m; gridDistX, gridDistY float[ny][nx] from
 * fimex_amd_griddistance_*; ap (Pa) and b: host double[nz] of the full levels; zs [ny][nx] orography in m; ps [nt][ny][nx] in Pa;
 * u, v (m/s), t (K) and w [nt][nz][ny][nx].  Everything is computed in double, floats promoted on read, with
 * R = 8.31432 / 0.0289644 and g = 9.80665:
 *   per column   mapRatioX = gridDistX / dx, mapRatioY = gridDistY / dy, rhx = 1 / mapRatioX, rhy = 1 / mapRatioY,
 *                rhxy = rhx * rhy, rdx_2 = 1 / (2 * dx), rdy_2 = 1 / (2 * dy)
 *   half levels  ah[0] = bh[0] = 0, ah[nz] = 0, bh[nz] = 1, for k = nz-1 .. 1: ah[k] = 2 * ap[k] - ah[k+1], bh[k] = 2 * b[k] - bh[k+1]
 *   levels k>=1  pm = ah[k] + bh[k] * ps, pp = ah[k+1] + bh[k+1] * ps, dp = pp - pm, dlnp = log(pp / pm), alfa = 1 - pm * dlnp / dp
 *   hydrostatic  from the surface upward, sum = zs * g: rt = R * t, z[k] = sum + rt * alfa, sum += rt * dlnp
 *   divergence   from k = 1 downward, sum = 0, in the interior 1 <= i < nx-1, 1 <= j < ny-1, with uu = mapRatioY * u * dp and
 *                vv = mapRatioX * v * dp of the neighbour cells:
 *                  div = rhxy * (rdx_2 * (uu[+1] - uu[-1]) + rdy_2 * (vv[+nx] - vv[-nx]))
 *                  w1 = R * t * (dlnp * sum + alfa * div) / dp,  w2 = rhx * rdx_2 * (z[+1] - z[-1]) + rhy * rdy_2 * (z[+nx] - z[-nx])
 *                  w = (float)((w1 + w2) / g),  sum = sum + div
 *                so sum never holds level k's own divergence when w of level k is taken, and level 0's is never added
 *   borders      rows j = 0 and ny-1 copy rows 1 and ny-2 for 1 <= i < nx-1, then columns i = 0 and nx-1 copy columns 1 and nx-2
 *                for every j; w at k = 0 is +0
 * NaN, non-positive pressures and zero distances are not treated specially: IEEE arithmetic decides.  The device's log is not
 * the host's (about 2^-51 relative), so w is the reference's within 2^-23 * |w| plus that error times the magnitude of the terms
 * that cancel in w1 + w2; almost every cell is bit-identical.
 * One divergence: for nx < 3, ny < 3 or nz < 1 the reference reads outside its arrays or uninitialised memory; these entries
 * return -1 with a message.  w must not overlap an input.  A scratch of (nz - 1) * ny * nx doubles is taken from the stream's
 * memory pool for the duration of the call.
 */
int fimex_amd_vertical_velocity_device(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* d_gridDistX,
                                       const float* d_gridDistY, const double* ap, const double* b, const float* d_zs, const float* d_ps,
                                       const float* d_u, const float* d_v, const float* d_t, float* d_w, void* stream);
int fimex_amd_vertical_velocity_host(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* gridDistX,
                                     const float* gridDistY, const double* ap, const double* b, const float* zs, const float* ps, const float* u,
                                     const float* v, const float* t, float* w);

/**
 * OmegaVerticalConverter::getDataSlice (src/CDMPressureConversions.cc:417-427) with mifi_omega_to_vertical_wind_f
 * (src/vertical_coordinate_transformations.c:195-209): w = ((mR_g * omega) * t) / p in float, mR_g = (float)(-8.31432 /
 * (9.80665 * 0.0289644)), p the level's pressure as float (what fimex_amd_vertical_levels_* would write), in the pressure unit
 * of omega (hPa and hPa/s in the reference).  omega, t and w [nt][pressure->nz][ny][nx]; w may be omega itself (the reference
 * converts in place) but must not overlap anything else.  The result is the reference's bit for bit.
 */
int fimex_amd_omega_to_vertical_wind_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_omega,
                                            const float* d_t, float* d_w, void* stream);
int fimex_amd_omega_to_vertical_wind_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* omega,
                                          const float* t, float* w);

/* ------------------------------------------------------------ grid merging (8f n8) */
/* CDMMerger's data path for float interpolation arrays (NaN = undefined), src/CDMMerger.cc:212-227:
 *   1  OI  = regrid(outer -> inner grid)              (CDMBorderSmoothing's interpolator; bilinear inside CDMMerger)
 *   2  S   = smooth(inner, OI)                        (CDMBorderSmoothing::getDataSlice)
 *   3  ST  = regrid(S -> target), OT = regrid(outer -> target)
 *   4  out = isnan(ST) ? OT : ST                      (CDMOverlay::getDataSlice)
 * Every step is the reference's arithmetic operation by operation; the results are the reference's bit for bit for variables
 * stored as float with scale 1 and offset 0 (a double variable is narrowed to float before the blend of step 2 here, after it in
 * the reference).  Packed variables, and every variable in its stored type, take the *_typed entries at the end of this block.
 * An x/y vector pair, which every interpolator of the merger rotates behind its regrid, takes fimex_amd_merge_apply_vector_device
 * behind the typed entries, a packed pair fimex_amd_merge_apply_vector_typed_device behind that (6.17). */
/**
 * CDMBorderSmoothing::getDataSlice (src/CDMBorderSmoothing.cc:129-139) with CDMBorderSmoothing_Linear::operator()
 * (src/CDMBorderSmoothing_Linear.cc:41-85) on [nz][ny][nx] slices: an undefined inner value gives the outer one
 * (useOuterIfInnerUndefined) or NaN, an undefined outer value the inner one; otherwise the outer value in the frame of
 * borderWidth cells, a linear blend over the next transitionWidth cells (the Euclidean distance in the corners) and the inner
 * value inside.  The cell classes follow the reference's size_t arithmetic, wrap-around included (grids narrower than
 * 2 * borderWidth + transitionWidth).  transitionWidth == 0, nx == 0 or ny == 0 is an error; nz == 0 does nothing.
 * out may be inner or outerOnInner itself, but must not overlap either otherwise.
 */
int fimex_amd_border_smooth_device(const float* d_inner, const float* d_outerOnInner, float* d_out, size_t nx, size_t ny, size_t nz,
                                   size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined, void* stream);
int fimex_amd_border_smooth_host(const float* inner, const float* outerOnInner, float* out, size_t nx, size_t ny, size_t nz,
                                 size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined);
/** CDMOverlay::getDataSlice (src/CDMOverlay.cc:82-86) on n values: top where it is defined, else base.  out may be either input
 *  itself, but must not overlap either otherwise; n == 0 does nothing. */
int fimex_amd_overlay_device(const float* d_top, const float* d_base, float* d_out, size_t n, void* stream);
int fimex_amd_overlay_host(const float* top, const float* base, float* out, size_t n);

typedef struct fimex_amd_merge_plan fimex_amd_merge_plan;
/**
 * The four steps as one plan.  It borrows three backward plans (nearest, bilinear or bicubic, each with its own method) that the
 * caller keeps alive as long as the merge plan: outer -> inner grid, (smoothed) inner -> target, outer -> target.  Refused:
 * transitionWidth == 0, forward plans, plans on different devices, shapes that do not chain (outerToInner.in == outerToTarget.in,
 * outerToInner.out == innerToTarget.in, innerToTarget.out == outerToTarget.out).
 */
int fimex_amd_merge_plan_create(const fimex_amd_regrid_plan* outerToInner, const fimex_amd_regrid_plan* innerToTarget,
                                const fimex_amd_regrid_plan* outerToTarget, size_t transitionWidth, size_t borderWidth,
                                int useOuterIfInnerUndefined, fimex_amd_merge_plan** plan);
int fimex_amd_merge_plan_destroy(fimex_amd_merge_plan* plan);
/**
 * CDMMerger::getDataSlice: inner [nz][iy][ix] and outer [nz][oy][ox] -> out [nz][ty][tx], steps 1-4 in two fused kernels that
 * evaluate the plans cell by cell only where a step reads them.  The smoothed inner field is stream-ordered
 * scratch.  out must not overlap the inputs; nz == 0 does nothing.  The _device form runs on the plans' device.
 */
int fimex_amd_merge_apply_device(const fimex_amd_merge_plan* plan, const float* d_inner, const float* d_outer, size_t nz, float* d_out,
                                 void* stream);
int fimex_amd_merge_apply_host(const fimex_amd_merge_plan* plan, const float* inner, const float* outer, size_t nz, float* out);
/** The same result by fimex_amd_regrid_apply_device three times and the two elementwise kernels, on temporaries: the cross-check
 *  and the yardstick of the fused kernels (as fimex_amd_regrid_apply_gather_device is for the staged ones). */
int fimex_amd_merge_apply_chain_device(const fimex_amd_merge_plan* plan, const float* d_inner, const float* d_outer, size_t nz, float* d_out,
                                       void* stream);

/* Grid merging on variables in their stored types: what CDMBorderSmoothing::getDataSlice and
 * CDMOverlay::getDataSlice compute on packed variables.  Both fields are read through getScaledDataSlice, each with its own
 * scale_factor, add_offset and _FillValue (ScaleValue to double, the fill value as NaN), blended in double, and packed by
 * convertDataType with the packing of the inner (top) variable, whose type the result has.  The three regrids are
 * fimex_amd_regrid_apply_typed_device on the raw counts:
 *   1  OI  = regridT(outer -> inner grid)                               in the outer's type
 *   2  S   = pack(smooth(unpack(inner), unpack(OI)))                    in the inner's type and packing
 *   3  ST  = regridT(S -> target), OT = regridT(outer -> target)
 *   4  out = pack(isnan(unpack(ST)) ? unpack(OT) : unpack(ST))          a defined value is unpacked and packed again
 * unpack and pack are what fimex_amd_convert_scaled_device computes (integer results through mifi_round and the wrapping casts,
 * not clamped; a fill value that does not exist in the input type matches nothing).  The host forms are declared in
 * fimex_amd_merge_typed_host.h. */
typedef struct fimex_amd_packing {
    int type;      /* fimex_amd_datatype, one of the ten numeric types */
    double fill;   /* _FillValue */
    double scale;  /* scale_factor */
    double offset; /* add_offset */
} fimex_amd_packing;
/**
 * fimex_amd_border_smooth_device on [nz][ny][nx] slices of innerPacking->type and outerPacking->type; d_out holds the inner's type in
 * the inner's packing.  d_out may be d_inner, and may be d_outerOnInner where the two element sizes agree; any other overlap is
 * refused, as are a NULL packing, a type without element size (NAT, STRING) and an inner fill value that is not representable in
 * the inner's type (fimex_amd_convert_scaled_device's rule).
 */
int fimex_amd_border_smooth_typed_device(const void* d_inner, const fimex_amd_packing* innerPacking, const void* d_outerOnInner,
                                         const fimex_amd_packing* outerPacking, void* d_out, size_t nx, size_t ny, size_t nz,
                                         size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined, void* stream);
/** fimex_amd_overlay_device on n values of topPacking->type and basePacking->type; d_out holds the top's type in the top's
 *  packing.  The same aliasing rule and refusals. */
int fimex_amd_overlay_typed_device(const void* d_top, const fimex_amd_packing* topPacking, const void* d_base,
                                   const fimex_amd_packing* basePacking, void* d_out, size_t n, void* stream);
/**
 * Steps 1-4 on d_inner [nz][iy][ix] of innerPacking->type and d_outer [nz][oy][ox] of outerPacking->type -> d_out [nz][ty][tx] of the
 * inner's type in the inner's packing.  *path (may be NULL; written as 0 before any check): 1 the two fused kernels ran (both
 * variables short, or both unsigned short, and the three buffers aligned to their element), 0 the chain below ran inside the
 * entry.  Same results either way.  d_out must not overlap the inputs; nz == 0 does nothing.  Runs on the plans' device.
 */
int fimex_amd_merge_apply_typed_device(const fimex_amd_merge_plan* plan, const void* d_inner, const fimex_amd_packing* innerPacking,
                                       const void* d_outer, const fimex_amd_packing* outerPacking, size_t nz, void* d_out, void* stream,
                                       int* path);
/** The same result as five launches on stream-ordered temporaries of the stored types: regridT three times and the two typed
 *  elementwise kernels.  The cross-check and the yardstick of the fused kernels. */
int fimex_amd_merge_apply_typed_chain_device(const fimex_amd_merge_plan* plan, const void* d_inner, const fimex_amd_packing* innerPacking,
                                             const void* d_outer, const fimex_amd_packing* outerPacking, size_t nz, void* d_out,
                                             void* stream);

/**
 * CDMMerger::getDataSlice on an x/y vector pair of float interpolation arrays, such as x_wind / y_wind.  Each of
 * the merger's three CDMInterpolators rotates the pair behind its regrid (src/CDMInterpolator.cc:259-283) with the matrices of
 * its CachedVectorReprojection: outerToInnerVec (R_oi) on the inner grid, innerToTargetVec (R_st) and outerToTargetVec (R_ot) on
 * the target.  rot(R; u, v) is fimex_amd_vector_reproject_values_device on one cell:
 *   1  (OIu, OIv) = rot(R_oi; regrid(outerU -> inner grid), regrid(outerV -> inner grid))
 *   2  Su = smooth(innerU, OIu), Sv = smooth(innerV, OIv)                      component by component
 *   3  (STu, STv) = rot(R_st; regrid(Su -> target), regrid(Sv -> target)),  (OTu, OTv) = rot(R_ot; regrid(outerU), regrid(outerV))
 *   4  outU = isnan(STu) ? OTu : STu, outV = isnan(STv) ? OTv : STv            component by component
 * A NaN in either regridded component, or in a cell's matrix, makes both rotated components NaN, so the next step falls back to
 * the inner value (step 2) or the outer pair (step 4).  Two fused kernels, a lane per cell, every plan entry decoded once for both
 * components; the smoothed pair is one stream-ordered scratch of 2 * nz * ix * iy floats.  The result is bit for bit that of the
 * chain below.  inner [nz][iy][ix], outer [nz][oy][ox], out [nz][ty][tx].  Refused: a NULL plan, a NULL vector plan (a pair that
 * no interpolator rotates is two scalar merges), a NULL buffer with nz > 0, a vector plan whose grid is not its regrid plan's
 * output grid or that lives on another device than the merge plan, a calling thread on another device, an output buffer that
 * overlaps any other buffer.  nz == 0 does nothing.  The host form is declared in fimex_amd_merge_vector_host.h.
 */
int fimex_amd_merge_apply_vector_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                        const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                        const float* d_innerU, const float* d_innerV, const float* d_outerU, const float* d_outerV, size_t nz,
                                        float* d_outU, float* d_outV, void* stream);
/** The same result step by step on stream-ordered temporaries: the pair regridded and rotated three times as
 *  fimex_amd_regrid_apply_vector_device does it, fimex_amd_border_smooth_device twice and fimex_amd_overlay_device twice.  The
 *  cross-check and the yardstick of the fused kernels. */
int fimex_amd_merge_apply_vector_chain_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                              const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                              const float* d_innerU, const float* d_innerV, const float* d_outerU, const float* d_outerV,
                                              size_t nz, float* d_outU, float* d_outV, void* stream);

/**
 * CDMMerger::getDataSlice on an x/y vector pair whose four fields -- inner u, inner v, outer u, outer v -- are in their stored
 * types, each with its own fimex_amd_packing: the typed merge and the vector merge above taken together.
 * regridRotT(plan, R; U, pU, V, pV) is fimex_amd_regrid_apply_vector_typed_device: both components read as raw counts with the
 * own fill value as NaN, regridded, rotated on the counts, each written back in its own type with its own fill value.
 *   1  (OIu, OIv) = regridRotT(outerToInner, R_oi; outerU, outerV)
 *   2  Su = pack_Iu(smooth(unpack_Iu(innerU), unpack_Ou(OIu))), Sv likewise with the v packings      blended in double
 *   3  (STu, STv) = regridRotT(innerToTarget, R_st; Su, Sv),  (OTu, OTv) = regridRotT(outerToTarget, R_ot; outerU, outerV)
 *   4  outU = pack_Iu(isnan(unpack_Iu(STu)) ? unpack_Ou(OTu) : unpack_Iu(STu)), outV likewise
 * The rotation acts on counts, as the reference's does: an add_offset is not rotated with the value, and two components with
 * different scales are rotated as if they had one.  An undefined count in either regridded component, or a NaN matrix cell, makes
 * both rotated components the fill value; a rotated count outside the type's range wraps (long -> int -> T), it is not clamped.
 * d_outU [nz][ty][tx] has inner u's type and packing, d_outV inner v's.  *path (may be NULL; written as 0 before any check): 1 the
 * two fused kernels ran (all four fields short, or all unsigned short; the six buffers aligned to 2 bytes; all four fill values
 * representable in the type), 0 the chain below ran inside the entry.  Same results either way.  Refused: a NULL plan, vector
 * plan or packing, a NULL buffer with nz > 0, a type without element size (NAT, STRING), an inner fill value that is not
 * representable in its type, a vector plan whose grid is not its regrid plan's output grid or that lives on another device than
 * the merge plan, a calling thread on another device, an output buffer that overlaps any other buffer (sizes counted in each
 * buffer's own element size).  nz == 0 does nothing.  The host form is declared in fimex_amd_merge_vector_typed_host.h.
 */
int fimex_amd_merge_apply_vector_typed_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                              const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                              const void* d_innerU, const fimex_amd_packing* innerUPacking, const void* d_innerV,
                                              const fimex_amd_packing* innerVPacking, const void* d_outerU, const fimex_amd_packing* outerUPacking,
                                              const void* d_outerV, const fimex_amd_packing* outerVPacking, size_t nz, void* d_outU, void* d_outV,
                                              void* stream, int* path);
/** The same result step by step on stream-ordered temporaries of the stored types: the pair regridded and rotated three times as
 *  fimex_amd_regrid_apply_vector_typed_device does it, fimex_amd_border_smooth_typed_device twice and
 *  fimex_amd_overlay_typed_device twice.  Serves all ten numeric types and components of different types.  The cross-check and
 *  the yardstick of the fused kernels. */
int fimex_amd_merge_apply_vector_typed_chain_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                                    const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                                    const void* d_innerU, const fimex_amd_packing* innerUPacking, const void* d_innerV,
                                                    const fimex_amd_packing* innerVPacking, const void* d_outerU,
                                                    const fimex_amd_packing* outerUPacking, const void* d_outerV,
                                                    const fimex_amd_packing* outerVPacking, size_t nz, void* d_outU, void* d_outV, void* stream);

/* ------------- scaled reads and writes, theta2T, humidity, accumulate (8f n9) */
/* The arithmetic around the entries above that the reference keeps in its readers and decorators: unpacking stored data
 * (scale_factor, add_offset, _FillValue, a linear unit change) into the floats n5-n8 take, packing results for the writers, the
 * theta2T and specific2relative converters of CDMPressureConversions, and accumulate / deAccumulate of CDMProcessor.  The
 * entries declared here only enqueue work on the stream and never synchronise it (the coefficient arrays of a level description
 * are host arrays, as everywhere).  Their *_host forms, on host buffers, are declared in fimex_amd_derived_host.h. */

/**
 * DataImpl<IN>::convertDataType -> ScaleValue<IN, OUT> (include/fimex/Utils.h:443-464, src/DataImpl.h:316-349) on n elements,
 * for every pair of the ten numeric fimex_amd_datatype values (NAT and STRING return -1).  With a = oldScale / newScale and
 * b = (oldOffset - newOffset) / newScale, taken once in double: an element equal to (IN)oldFill, or NaN for a floating IN, gives
 * (OUT)newFill; any other gives data_caster<OUT, double>(a * in + b) with the product and the sum in double: for an integer OUT
 * static_cast<OUT>((int)lround(.)), half away from zero, with the int's wrap-around (and 0 beyond the range of long, DESIGN.md
 * divergence D6), for float and double a plain cast.
 *
 * getScaledDataSliceInUnit(var, unit, t) maps onto it as CDMReader::scaleDataOf (src/CDMReader.cc:164-179) does, a linear unit
 * change (unitScale, unitOffset: new = unitScale * old + unitOffset) folded into the arguments:
 *   oldFill = _FillValue, oldScale = scale_factor * unitScale, oldOffset = unitScale * add_offset + unitOffset,
 *   outType = FIMEX_AMD_CDM_DOUBLE, newFill = NaN, newScale = 1, newOffset = 0.
 * outType FIMEX_AMD_CDM_FLOAT gives what ->asFloat() of that slice holds (the input of every n5-n8 entry), bit for bit: the same
 * double rounded to float once.  Non-linear unit conversions (ScaleValueUnits) are not covered.
 * The writers' packing is the same call with the variable's own fill, scale and offset as the new* arguments.
 *
 * Two divergences.  Where static_cast<IN>(oldFill) is undefined in the reference (a NaN or a value beyond the range of an integer
 * IN, a finite value beyond the range of float) the data has no fill value here: no element compares equal.  A newFill that OUT
 * cannot hold in the same sense returns -1.
 * out may be in itself when both types have the same size; any other overlap returns -1.  n == 0 does nothing.
 * Throughput depends on the two pointers: 16-byte accesses need a common element offset below 16 at which both are 16-byte
 * aligned (always so for two 16-byte aligned buffers, or two buffers shifted by the same number of elements); otherwise every
 * element goes on its own, which is correct and slower.
 */
int fimex_amd_convert_scaled_device(const void* d_in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType,
                                    double newFill, double newScale, double newOffset, void* d_out, void* stream);

/**
 * ThetaTemperatureConverter::getDataSlice (src/CDMPressureConversions.cc:226-245), all in float:
 * T = ((theta + addOffset) * powf(p * (1 / 1000.f), Rcp)) - addOffset, Rcp = (float)(8.31432 / 0.0289644) / 1004.f, p the level's
 * pressure as float in hPa (what fimex_amd_vertical_levels_* would write; a formula kind is evaluated per column, no pressure field
 * is needed), addOffset the add_offset attribute of theta.  theta and T [nt][pressure->nz][ny][nx]; T may be theta itself (the
 * reference converts in place) but must not overlap anything else.  The device's powf is not the host's: T is within
 * 3 * 2^-23 * |(theta + addOffset) * powf(.)| of the reference's.
 */
int fimex_amd_theta_to_temperature_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_theta,
                                          float addOffset, float* d_T, void* stream);

/**
 * HumidityConverter::getDataSlice (src/CDMPressureConversions.cc:313-333): relative humidity packed as short with scale factor
 * 1 / 25000 from specific humidity q (1), air temperature T (K) and the level's pressure p as float in hPa, by
 * mifi_specific_to_relative_humidity (src/vertical_coordinate_transformations.c:114-141):
 *   es = (float)(610.78f * exp((17.269f * (T - 273.16f)) / (T - 35.86f)))   the argument in float, exp and the product in double
 *   rh = (float)(100. * q * p / (es * 0.622))                               in double, then clamped to [0, 100] (NaN stays)
 *   packed = (short)(25000.f * rh + 0.5)                                    a float product, + 0.5 in double, truncation
 * Where a short cannot hold the result the reference is undefined; written here is what its x86-64 build yields: the value
 * truncated to int32, of which the low 16 bits are kept (rh = 1.4 gives -30536, rh = 3 gives 9464), and 0 for NaN.
 * q, T and rh [nt][pressure->nz][ny][nx]; rh must not overlap an input.  The device's exp is not the host's: an element differs
 * from the reference's by at most one count, and almost none does.
 */
int fimex_amd_specific_to_relative_humidity_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_q,
                                                   const float* d_T, short* d_rh, void* stream);

/**
 * The accumulation of CDMProcessor::getDataSlice (src/CDMProcessor.cc:470-491, :534-558) for nt positions of the unlimited
 * dimension, firstPos .. firstPos + nt - 1: in [nt][n] elements of cdmType, read as Data::asDouble() (a cast, no fill value
 * handling), out double[nt][n].  In the order a writer pulling positions 0, 1, 2, ... gets from the reference's slice cache:
 *   acc[0] = in[0] (its NaN kept), acc[1] = in[1] + nan0(in[0]), acc[t] = in[t] + acc[t-1]
 * where nan0 replaces NaN by 0 and applies to position 0 only, where it is the addend.  prev: double[n] holding acc[firstPos - 1],
 * required when firstPos > 0 and ignored otherwise (for firstPos == 1 it is position 0 and gets nan0).  Bit for bit.
 * out must not overlap in or prev; n == 0 or nt == 0 does nothing.
 */
int fimex_amd_accumulate_device(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* d_prev, double* d_out,
                                void* stream);
/**
 * The deaccumulation (:560-578): out[0] = in[0], out[t] = in[t] - in[t-1] with nan0 on in[0] where it is the subtrahend.
 * prev: in[firstPos - 1], n elements of cdmType, required when firstPos > 0.  Everything else as above.
 */
int fimex_amd_deaccumulate_device(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* d_prev, double* d_out,
                                  void* stream);

/* ------------------------------------------- time axis and quality mask (8f n10) */
/* The *_host forms of the two *_device entries below are declared in fimex_amd_time_quality_host.h. */

/**
 * The slice mapping of CDMTimeInterpolator::changeTimeAxis (src/CDMTimeInterpolator.cc:161-188) on doubles: for every new time the
 * pair (t1[i], t2[i]) of old positions it is blended from.  oldTimes: the old times in the new unit, strictly ascending (refused
 * otherwise, as is nOld == 0).  Per new time pos = lower_bound(oldTimes + lastPos, oldTimes + nOld, x), with lastPos the pos of
 * the step before (so a new axis that runs backwards gives what the reference gives); pos == nOld becomes nOld - 1; t2 = pos and
 * t1 = pos - 1, except at pos == 0, where t1 = 0 and t2 = 1 if there is a second old time.  One old time gives (0, 0).
 * Host arrays throughout; runs on the CPU and initialises nothing on a device.  nNew == 0 does nothing.
 */
int fimex_amd_time_mapping(const double* oldTimes, size_t nOld, const double* newTimes, size_t nNew, size_t* t1, size_t* t2);

/** output steps per launch of fimex_amd_time_interpolate_device, and per chunk: a chunk re-reads the first pair it needs */
#define FIMEX_AMD_TIME_LAUNCH_STEPS 128
#define FIMEX_AMD_TIME_CHUNK_STEPS 32

/**
 * CDMTimeInterpolator::getDataSlice (src/CDMTimeInterpolator.cc:88-136) for every position of the new time axis in one pass:
 * d_in [nOld][n] elements of cdmType (any of the ten numeric types), d_out float[nNew][n].  Output step i is
 * mifi_get_values_linear_weak_extrapol_f (src/interpolation.c:1085-1109) on Data::asFloat() (a cast per element, no scale, no fill
 * value handling) of the slices t1[i] and t2[i] of fimex_amd_time_mapping, with a = oldTimes[t1], b = oldTimes[t2], x = newTimes[i]:
 *   f = (float)((x - a) / (b - a)), 0 where a == b
 *   f == 0: a copy of A (a NaN in B does not leak in);  f == 1: a copy of B;  -1 <= f <= 2: A + f * (B - A) in float, uncontracted;
 *   otherwise MIFI_UNDEFINED_F.  Bit for bit.
 * The time arrays are host arrays and are free on return; the call only enqueues on `stream`.  A new axis that never runs backwards
 * reads every input slice once per FIMEX_AMD_TIME_LAUNCH_STEPS output steps at most.  nOld must fit 32 bits.  d_out must not
 * overlap d_in.  The times are checked first; after that n == 0 or nNew == 0 does nothing.
 */
int fimex_amd_time_interpolate_device(const void* d_in, int cdmType, size_t n, const double* oldTimes, size_t nOld, const double* newTimes,
                                      size_t nNew, float* d_out, void* stream);

/** The rules of CDMQualityExtractor (the "use" attribute of its configuration, or a list of status values). */
typedef enum fimex_amd_quality_mode {
    FIMEX_AMD_QUALITY_VALUES = 0, /* keep cells whose status is one of values[] */
    FIMEX_AMD_QUALITY_ALL,        /* keep every defined status */
    FIMEX_AMD_QUALITY_MAX,        /* "max:<limit>": a status above limit is undefined */
    FIMEX_AMD_QUALITY_MIN,        /* "min:<limit>": a status below limit is undefined */
    FIMEX_AMD_QUALITY_HIGHEST,    /* keep cells whose status is the largest defined status of the slice */
    FIMEX_AMD_QUALITY_LOWEST      /* ... the smallest */
} fimex_amd_quality_mode;

/**
 * CDMQualityExtractor::getDataSlice (src/CDMQualityExtractor.cc:239-391), in place: d_data[i] = fillValue wherever the status of
 * cell i % nStatus fails the rule.  d_data: nData elements of dataType, d_status: nStatus elements of statusType, read as
 * Data::asDouble(); both any of the ten numeric types.  nData must be a positive multiple of nStatus: the status repeats along
 * the slow dimensions (:377-385).  Any other ratio is refused; the reference warns and passes the data on, which is the caller's
 * part.  nData == 0 does nothing.
 *   VALUES: masked where the status is none of values[nValues] (a host array; an empty list or a NaN in it is refused).
 *           validMin, validMax and statusFill are ignored, as in the reference (:285-288).
 *   the other modes: the status is undefined below validMin, above validMax and where it equals statusFill (NaN: no such bound),
 *           then where the mode's rule says so (:304-361); masked where it is undefined.
 *   A NaN status masks in every mode (:380).
 * HIGHEST and LOWEST do what include/fimex/CDMQualityExtractor.h documents, not what findDefinedExtreme (:219-237) does
 * (DESIGN.md divergence D8); with no defined status every cell is masked.
 * fillValue goes through data_caster<C, double> (include/fimex/Utils.h:85-115): rounded half away from zero to int and cast for an
 * integer type, a plain cast otherwise.  A fill the type cannot hold that way (the cast does not give the rounded value back; beyond
 * the range of float) is refused.
 * d_status may be d_data itself with one type and nStatus == nData (the reference's own-status case); any other overlap is refused.
 * The call only enqueues on `stream`; values[] is free on return.
 */
int fimex_amd_quality_mask_device(void* d_data, int dataType, size_t nData, const void* d_status, int statusType, size_t nStatus, int mode,
                                  const double* values, size_t nValues, double limit, double validMin, double validMax, double statusFill,
                                  double fillValue, void* stream);

/* ------------------------------------------------------- extraction (8f n11) */
/* CDMExtractor's data path (src/CDMExtractor.cc): a variable with some dimensions reduced to picked positions, read through a
 * SliceBuilder window, and the index computations behind reduceTime / reduceVerticalAxis and reduceLatLonBoundingBox. */
#define FIMEX_AMD_EXTRACT_MAX_DIMS 8

typedef struct fimex_amd_extract_dim {
    size_t length;            /* length of the dimension in the source */
    int reduced;              /* 0: not in dimSlices_, every position is taken; positions and nPositions are ignored */
    const size_t* positions;  /* host array, strictly ascending, every entry < length; may be NULL when nPositions == 0 */
    size_t nPositions;
    size_t start, size;       /* the SliceBuilder window in the reduced dimension: start + size <= (reduced ? nPositions : length) */
} fimex_amd_extract_dim;      /* dims[0] is the fastest dimension */

typedef struct fimex_amd_extract_info {
    size_t inElements, outElements;
    size_t kernelDims;          /* dimensions left after folding lengths of 1 and merging whole neighbours (0: nothing to move) */
    size_t fastestRuns;         /* contiguous source runs of one output row of the merged fastest dimension */
    int referenceOrderDiffers;  /* divergence D9: the reference's joinSlices emits these elements in another order */
} fimex_amd_extract_info;

/** Opaque, immutable extraction plan: the offset tables of one variable's reduction, resident in HBM. */
typedef struct fimex_amd_extract_plan fimex_amd_extract_plan;

/**
 * Checks a reduction and describes the plan it gives; runs on the CPU and initialises nothing on a device.  Refused: nDims == 0
 * or above FIMEX_AMD_EXTRACT_MAX_DIMS, a dimension of length 0 with a non-empty window, positions that are not strictly ascending
 * or reach the length, a window beyond the reduced length, NULL where an array is needed, a source of more elements than size_t
 * counts.  referenceOrderDiffers: the output holds an element, some reduced dimension's window is cut into more than one run of
 * neighbouring positions, and a slower dimension that is not reduced has a window longer than 1 (src/CDMExtractor.cc:96-179 then
 * emits run-major data under a row-major shape; the apply entries below always give the row-major array).
 */
int fimex_amd_extract_describe(const fimex_amd_extract_dim* dims, size_t nDims, fimex_amd_extract_info* info);
/** The same checks, then the tables are built and uploaded to the calling thread's device.  dims and the position arrays are free
 *  on return. */
int fimex_amd_extract_plan_create(const fimex_amd_extract_dim* dims, size_t nDims, fimex_amd_extract_plan** plan);
int fimex_amd_extract_plan_destroy(fimex_amd_extract_plan* plan);
int fimex_amd_extract_plan_info(const fimex_amd_extract_plan* plan, fimex_amd_extract_info* info);
/**
 * CDMExtractor::getDataSlice_ (src/CDMExtractor.cc:96-179) for one variable.  With p_d(i) = positions_d[start_d + i] for a reduced
 * dimension and start_d + i otherwise, out is the row-major array out[i_{n-1}]...[i_0] = in[p_{n-1}(i_{n-1})]...[p_0(i_0)] of
 * info.outElements elements; in holds info.inElements elements.  cdmType: any of the ten numeric fimex_amd_datatype values; only
 * its element size matters, bytes are moved and never interpreted.  Both pointers must be aligned to the element size; out must
 * not overlap in.  outElements == 0 does nothing and accepts NULL pointers.  A plan is immutable: apply may run from several
 * threads and streams at once.  The call only enqueues on `stream` and must run on the plan's device.
 */
int fimex_amd_extract_apply_device(const fimex_amd_extract_plan* plan, const void* d_in, int cdmType, void* d_out, void* stream);
/**
 * The index arithmetic of CDMExtractor::reduceAxes (src/CDMExtractor.cc:369-406) on a 1-D axis already in the unit of startVal and
 * endVal (units.convert stays with the caller): delta = 1e-5, or 0.01 * |axis[0] - axis[1]| when these differ; a descending axis
 * (axis[0] > axis[1]) is searched reversed; start = lower_bound(startVal - delta), end = upper_bound(endVal + delta),
 * size = max(end - start, 0), and start = n - size - start on a descending axis.  n == 0 gives (0, 0).  A NaN in the axis or
 * in the bounds is refused.  Runs on the CPU and initialises nothing on a device.
 */
int fimex_amd_extract_axis_range(const double* axis, size_t n, double startVal, double endVal, size_t* start, size_t* size);
/* The *_host form of the apply and the bounding box on host axes are declared in fimex_amd_extract_host.h. */

/* ----------------------------------- plan building across projections (8f n2) */
/* The reference calls PROJ.4 (pj_init_plus / pj_transform) here; this library carries its own projections:
 * latlong/longlat, stere, lcc, merc, tmerc, etmerc, utm, laea, aea, geos, omerc, sinu, cea, ortho, aeqd, nsper, ob_tran with o_proj=longlat (radians at this boundary for
 * geographic and rotated coordinates, as PROJ.4's legacy API), on a sphere (+R, +a +e=0, +ellps=sphere) or an ellipsoid
 * (+ellps, +datum=WGS84|NAD83, +a with +b/+rf/+f/+e/+es).  Three- and seven-parameter datum shifts (+towgs84, +datum=WGS84|NAD83|GGRS87|potsdam)
 * are applied as pj_transform does; strings that need a grid shift, +units, +pm, +axis or another projection make the call
 * fail with a message. */
/** mifi_project_values, include/fimex/interpolation.h / src/interpolation.c:1158-1197: n points in place. */
int fimex_amd_project_values_host(const char* proj_input, const char* proj_output, double* in_out_x_vals, double* in_out_y_vals, size_t num);
int fimex_amd_project_values_device(const char* proj_input, const char* proj_output, double* d_x_vals, double* d_y_vals, size_t num, void* stream);
/** mifi_project_axes, src/interpolation.c:1199-1244: the [iy][ix] mesh of two host axes, transformed; the device form
 *  leaves the two fields in device memory (feed fimex_amd_points2position_device / fimex_amd_regrid_plan_create_device). */
int fimex_amd_project_axes_host(const char* proj_input, const char* proj_output, const double* in_x_axis, const double* in_y_axis,
                                size_t ix, size_t iy, double* out_xproj_axis, double* out_yproj_axis);
int fimex_amd_project_axes_device(const char* proj_input, const char* proj_output, const double* in_x_axis, const double* in_y_axis,
                                  size_t ix, size_t iy, double* d_out_xproj_axis, double* d_out_yproj_axis, void* stream);
/** mifi_get_vector_reproject_matrix, src/interpolation.c:719-788: matrix[4*ox*oy] = (cos, sin, -sin, phi) of the local
 *  rotation from proj_input to proj_output on the mesh of the output axes (degrees for FIMEX_AMD_LONGITUDE /
 *  FIMEX_AMD_LATITUDE axis types, as the reference).  Host or device destination. */
int fimex_amd_get_vector_reproject_matrix_host(const char* proj_input, const char* proj_output, const double* out_x_axis,
                                               const double* out_y_axis, int out_x_axis_type, int out_y_axis_type,
                                               size_t ox, size_t oy, double* matrix);
int fimex_amd_get_vector_reproject_matrix_device(const char* proj_input, const char* proj_output, const double* out_x_axis,
                                                 const double* out_y_axis, int out_x_axis_type, int out_y_axis_type,
                                                 size_t ox, size_t oy, double* d_matrix, void* stream);
/** mifi_get_vector_reproject_matrix_field, src/interpolation.c:657-717: the [oy][ox] mesh is given as two fields in the
 *  INPUT projection (CDMProcessor's rotation to lat/lon, src/CDMProcessor.cc:123-136). */
int fimex_amd_get_vector_reproject_matrix_field_host(const char* proj_input, const char* proj_output, const double* in_x_field,
                                                     const double* in_y_field, size_t ox, size_t oy, double* matrix);
/** mifi_get_vector_reproject_matrix_points, src/interpolation.c:607-655: on points in the OUTPUT projection (m or rad),
 *  finite difference of 100 m (inputIsMetric) or 1e-5 rad. */
int fimex_amd_get_vector_reproject_matrix_points_host(const char* proj_input, const char* proj_output, int inputIsMetric,
                                                      const double* out_x_points, const double* out_y_points, size_t on, double* matrix);
/** Projection::isDegree (src/coordSys/Projection.cc): 1 for geographic and rotated lat/lon strings, 0 otherwise, -1 on error. */
int fimex_amd_projection_is_degree(const char* proj);

/* ------------------------------- coordinate-based nearest neighbour plans (8f n3) */
/** fastTranslatePointsToClosestInputCell with getGridDistance, src/CDMInterpolator.cc:1069-1217 (MIFI_INTERPOL_COORD_NN):
 *  pointsOnXAxis / pointsOnYAxis hold longitude / latitude (rad) of every target cell on entry and the x / y index of the
 *  closest source cell (as doubles, -1 when none lies within the grid's region of influence) on return; lonVals / latVals:
 *  the source grid's coordinates in rad, [orgYDimSize][orgXDimSize], NaN = undefined.  The result is the plan of
 *  fimex_amd_regrid_plan_create(MIFI_INTERPOL_COORD_NN, ...). */
int fimex_amd_coord_nearest_host(double* pointsOnXAxis, double* pointsOnYAxis, size_t nPoints,
                                 const double* lonVals, const double* latVals, size_t orgXDimSize, size_t orgYDimSize);
int fimex_amd_coord_nearest_device(double* d_pointsOnXAxis, double* d_pointsOnYAxis, size_t nPoints,
                                   const double* d_lonVals, const double* d_latVals, size_t orgXDimSize, size_t orgYDimSize, void* stream);
/** flannTranslatePointsToClosestInputCell, src/CDMInterpolator.cc:991-1067 (MIFI_INTERPOL_COORD_NN_KD): closest source
 *  cell within maxDist metres (chord on a sphere of MIFI_EARTH_RADIUS_M), -1000 when none. */
int fimex_amd_coord_kdtree_host(double maxDist, double* pointsOnXAxis, double* pointsOnYAxis, size_t nPoints,
                                const double* lonVals, const double* latVals, size_t orgXDimSize, size_t orgYDimSize);
int fimex_amd_coord_kdtree_device(double maxDist, double* d_pointsOnXAxis, double* d_pointsOnYAxis, size_t nPoints,
                                  const double* d_lonVals, const double* d_latVals, size_t orgXDimSize, size_t orgYDimSize, void* stream);
/** getGridDistance, src/CDMInterpolator.cc:1069-1141: the region of influence (rad) COORD_NN derives from the source grid. */
int fimex_amd_grid_distance_host(const double* lonVals, const double* latVals, size_t orgXDimSize, size_t orgYDimSize, double* maxGridDistance);

/* ------------------------------------------------------------- diagnostics */
/** The scan-order double sums the fills start with (src/interpolation.c:1256-1264 sum of the defined values, mode 0;
 *  :1288-1299 sum of |v - average|, mode 1; mode 2 only counts), on n device floats: exactly the value the reference's
 *  sequential loop accumulates.  algo 0 walks the additions one by one, algo 1 evaluates them binade-parallel (the
 *  fills' default); both must agree bit for bit -- this entry exists so that tests can check that directly. */
int fimex_amd_scan_sum_device(const float* d_values, size_t n, int mode, double average, int algo,
                              double* sum, size_t* nUndefined, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FIMEX_AMD_H_ */
