// Regrid and rotation plans as they live in HBM.
//
// The reference keeps, per output cell, two doubles (fractional source position,
// include/fimex/CachedInterpolation.h:108-109) and re-derives floor / fraction /
// border class for every cell of every call.  Here that derivation runs once, on the
// GPU, when the plan is created; the apply kernels read a compact structure-of-arrays
// form that reproduces the reference's arithmetic bit for bit:
//
//   nearest   pos[n]            u32  source offset inside a slice, kInvalidPos = undefined
//   bilinear  pos[n], xf[n], yf[n]   u32 + 2 x f32.  xf/yf are the fractions already rounded
//             to float exactly as src/interpolation.c:885,888 does.  A set sign bit in xf
//             (yf) marks "nearest neighbour in x (y)", i.e. the border branches of
//             interpolation.c:903-948; pos then already points at the rounded cell.
//   bicubic   pos[n], xfd[n], yfd[n] u32 + 2 x f64 (double fractions, interpolation.c:971,973);
//             pos is the (x0-1, y0-1) corner of the 4x4 stencil.
//   forward   offsets[nOut+1], src[nMapped]   CSR inverse of the reference's per-source-cell
//             target index (src/CachedForwardInterpolation.cc:72-73), buckets in source scan
//             order so that sums add in the reference's push_back order.
#pragma once

#include "backward_dispatch.hpp"
#include "blend_math.hpp"
#include "common.hpp"
#include "staged_layout.hpp"

#include <functional>
#include <mutex>

namespace fimex_amd {

constexpr uint32_t kInvalidPos = 0xFFFFFFFFu;
// source slices are addressed with 32-bit cell offsets (and 32-bit byte offsets in the kernels)
constexpr size_t kMaxSliceCells = (size_t(1) << 30) - 1;

// (PlanKind: backward_dispatch.hpp)
enum class Aggregate : int { Sum = 0, Mean = 1, Median = 2, Max = 3, Min = 4 };

}  // namespace fimex_amd

namespace fimex_amd {
static_assert(layout::kXcds == (uint32_t)kXcds, "staged_layout.hpp deals workgroups to the XCDs of common.hpp");

// LDS-staged form of a bilinear / bicubic plan (staged.hip): per tile the source row segments to stream into
// LDS, per output cell the 16-bit LDS offsets of its stencil rows; the fractions are those of the gather plan.
struct StagedPlan {
    bool valid = false;
    uint32_t tileW = 0, tileH = 0, per = 0, kmax = 0, tilesX = 0, nTiles = 0;
    size_t stagedCells = 0;  // source cells streamed per slice (16-byte granules, all tiles)
    DeviceArray<uint32_t> tileRows;
    DeviceArray<uint2> tileHdr;
    DeviceArray<uint32_t> ldsA, ldsB;  // LDS offsets of stencil rows 0|1 (and 2|3 for bicubic), 16 bits each
};

// Second LDS-staged form (staged2_plan.hip builds it, staged2.hip and staged2_typed.hip run it): tiles of one height and varying width (narrower where the source footprint of an
// output cell is larger, so that every tile fits the same LDS budget), workgroups of 256-1024 threads, and per tile the
// list of 16-byte source chunks itself instead of row segments.  StagedTile and the rules that cut the tiles: staged_layout.hpp.
struct Staged2Plan {
    bool valid = false;
    uint32_t nt = 0, per = 0, kmax = 0, tileH = 0, tileWMax = 0, nTiles = 0, gridX = 0, ldsBytes = 0, depth = 2;
    size_t stagedCells = 0, totalChunks = 0;
    DeviceArray<StagedTile> tiles;
    DeviceArray<uint32_t> order;     // workgroup -> tile, ~0u = none (tile rows dealt to the XCDs in stripes)
    DeviceArray<uint32_t> orderChunkXcd;  // the nTiles entries every XCD walks in the chunk-per-XCD order (chunk_xcd_order)
    DeviceArray<uint32_t> chunkOff;  // source cell offset of every chunk inside a slice
    DeviceArray<uint32_t> ldsA, ldsB;
};

// forward_tiled.hip: the LDS-staged form of a forward plan whose buckets are long (tiles of 64 targets, one wave each)
struct ForwardTile {
    uint32_t chunkBase;  // first entry of the tile in chunkOff
    uint32_t nChunks;    // ~0u: the tile's buckets are spread too far for LDS, it reads from memory
    uint32_t stepBase;   // first entry of the tile in steps
    uint32_t maxLen;     // longest bucket of the tile; 0: every target of the tile is empty
};
struct ForwardTiles {
    bool valid = false;
    uint32_t tw = 0, th = 0, tilesX = 0, nTiles = 0, slotChunks = 0, groups = 0;  // groups: eight-step groups of the longest bucket
    uint32_t cellBytes = 4;  // element size of the slices this form stages: 4 (float), 2 or 1 (stored types)
    size_t stagedTiles = 0, directTiles = 0, stagedChunks = 0;
    DeviceArray<ForwardTile> tiles;
    DeviceArray<uint32_t> chunkOff;      // source cell index of every 16-byte chunk a tile stages, row by row
    DeviceArray<unsigned short> steps;   // LDS position of every cell of every bucket, in the order the lanes of a tile walk them
};
}  // namespace fimex_amd

struct fimex_amd_regrid_plan {
    int funcType = 0;
    int device = 0;
    fimex_amd::PlanKind kind = fimex_amd::PlanKind::Nearest;
    bool bicubicFast = false;  // FIMEX_AMD_BICUBIC_FAST: float fused multiply-adds in the LDS-staged bicubic kernel
    size_t inX = 0, inY = 0, outX = 0, outY = 0;

    // backward plans
    fimex_amd::DeviceArray<uint32_t> pos;
    fimex_amd::DeviceArray<float> xf, yf;
    fimex_amd::DeviceArray<double> xfd, yfd;
    fimex_amd::StagedPlan staged;
    fimex_amd::Staged2Plan staged2;
    // Second workgroup shape of the same plan (bilinear: 512 threads on 256 x 8 tiles next to 1024 threads on 512 x 8; bicubic in float
    // arithmetic: 256 threads on 128 x 8 next to 512 on 256 x 8), same results
    // bit for bit.  Which one is faster depends on the device at hand and on the batch length;
    // fimex_amd_regrid_plan_tune_device times both on the caller's buffers and sets useAlt.
    fimex_amd::Staged2Plan staged2Alt;
    int useAlt = 0;
    size_t planBytesShape[2] = {0, 0};  // info.planBytes with either shape
    // The launch order of float batches long enough for it (chunk_xcd_chunk_count, staged_layout.hpp): 0 an XCD owns whole tiles,
    // 1 an XCD owns z chunks of every tile.  Same results bit for bit; fimex_amd_regrid_plan_tune_device times the second one too
    // and keeps it where it is clearly faster (info.launchOrder says which).
    int chunkXcd = 0;

    // The second staged form for slices of 1- and 2-byte stored types (staged2_typed.hip): built from this plan's own arrays on the
    // first typed apply of that element size, under the mutex (plans are shared by threads; everything else is immutable).
    struct TypedForms {
        std::mutex mtx;
        bool tried[2] = {false, false};  // [0] 2-byte elements, [1] 1-byte elements
        fimex_amd::Staged2Plan form[2];
    };
    mutable TypedForms typed2;

    // forward plans
    fimex_amd::Aggregate aggregate = fimex_amd::Aggregate::Sum;
    bool undefAggr = false;
    fimex_amd::DeviceArray<uint32_t> offsets, src;
    fimex_amd::ForwardTiles fwdTiles;
    // the same for slices of 2- and 1-byte stored types, built on the first typed apply of that element size (see TypedForms)
    struct FwdTypedForms {
        std::mutex mtx;
        bool tried[2] = {false, false};
        fimex_amd::ForwardTiles form[2];
    };
    mutable FwdTypedForms fwdTyped;

    fimex_amd_plan_info info{};
};

struct fimex_amd_vector_plan {
    int device = 0;
    size_t ox = 0, oy = 0;
    fimex_amd::DeviceArray<double2> cossin;  // (m0, m1) of the reference matrix
    fimex_amd::DeviceArray<double> phi;      // m3
};

// CDMMerger's data path (merge.hip): three backward plans borrowed from the caller and the parameters of
// CDMBorderSmoothing_LinearFactory
struct fimex_amd_merge_plan {
    int device = 0;
    const fimex_amd_regrid_plan *outerToInner = nullptr, *innerToTarget = nullptr, *outerToTarget = nullptr;
    size_t transitionWidth = 5, borderWidth = 2;
    bool useOuter = true;  // setUseOuterIfInnerUndefined
};

namespace fimex_amd {

// backward_plan.hip: classification, and the launches of the kernel that backward_dispatch.hpp names for a call.
// dispatch_switches is the only reader of the eight experiment switches of that rule; a caller fills them once and asks the rule.
dispatch::Switches dispatch_switches();
inline dispatch::PlanFacts plan_facts(const fimex_amd_regrid_plan& plan)
{
    return {plan.kind, plan.funcType, plan.bicubicFast, plan.staged.valid, plan.staged2.valid, plan.inX, plan.inY, plan.outX, plan.outY};
}
inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }
void build_backward_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream);
void launch_backward_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
// the LaunchOrder (staged_layout.hpp) of launch_backward_apply's launch of nz slices; -1: not a float launch of the second staged form
int backward_launch_order(const fimex_amd_regrid_plan& plan, size_t nz);
bool launch_typed_apply(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                        hipStream_t stream);
// A list of variables, variable i an array of nz[i] slices of its own, through the second staged form's list kernels
// (staged2_list.hip, staged2_list_typed.hip) in launches of at most kSliceListMaxVars variables.  false, and nothing launched: the
// rule (float_list / typed_list, on the SUM of nz[]) or the list kernels' shapes say no; the caller runs the variables one by one.
bool launch_backward_apply_list(const fimex_amd_regrid_plan& plan, size_t nvar, const float* const* d_in, const size_t* nz, float* const* d_out,
                                hipStream_t stream);
bool launch_typed_apply_list(const fimex_amd_regrid_plan& plan, size_t nvar, const void* const* d_in, int cdmType, const size_t* nz,
                             const double* badValue, void* const* d_out, hipStream_t stream);
// gather.hip: the per-lane gather kernel on float slices and on stored types
void launch_backward_gather(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
void launch_typed_gather(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                         hipStream_t stream);

// staged.hip
bool build_staged_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream);
void launch_staged_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
void launch_staged_apply_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                               hipStream_t stream);

// staged2_plan.hip
bool build_staged2_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream);
// staged2.hip
void launch_staged2_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
int staged2_float_launch_order(const fimex_amd_regrid_plan& plan, size_t nz);  // the LaunchOrder launch_staged2_apply runs nz slices in
// staged2_list.hip, staged2_list_typed.hip: one launch on the slices of nvar <= kSliceListMaxVars variables; `serves`: the list
// kernels exist for the workgroup shape the plan's launches run (and, stored types, the plan has a form for the type)
bool staged2_list_serves(const fimex_amd_regrid_plan& plan);
void launch_staged2_apply_list(const fimex_amd_regrid_plan& plan, const dispatch::Switches& sw, size_t nvar, const float* const* d_in,
                               const size_t* nz, float* const* d_out, hipStream_t stream);
bool staged2_list_typed_serves(const fimex_amd_regrid_plan& plan, int cdmType, hipStream_t stream);
void launch_staged2_apply_list_typed(const fimex_amd_regrid_plan& plan, size_t nvar, const void* const* d_in, int cdmType, const size_t* nz,
                                     const double* badValue, void* const* d_out, hipStream_t stream);
// staged2_vector.hip: both components of a vector pair regridded and rotated in one launch (the rule: vector_fused)
void launch_staged2_apply_vector(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const float* d_u, const float* d_v, size_t nz,
                                 float* d_uOut, float* d_vOut, hipStream_t stream);
// staged2_typed.hip; false, nothing launched: the plan has no form for slices of this element size (staged2_typed_form)
bool launch_staged2_apply_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                                hipStream_t stream);

// staged2_vector_typed.hip: a vector pair on its stored type (short / unsigned short, both components in one type) regridded and
// rotated in one launch (the rule: vector_typed_fused); false, nothing launched: the plan has no 2-byte form
bool launch_staged2_apply_vector_typed(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const void* d_u, const void* d_v,
                                       int cdmType, double uBad, double vBad, size_t nz, void* d_uOut, void* d_vOut, hipStream_t stream);

// forward_plan.hip
void build_forward_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream);
// forward.hip (the medians of medium buckets: forward_median.hip, declared in forward.hpp)
void launch_forward_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);

// forward_tiled.hip
void build_forward_tiles(fimex_amd_regrid_plan& plan, hipStream_t stream);
bool launch_forward_tiled(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
bool launch_forward_tiled_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                                hipStream_t stream);

// vector.hip
void build_vector_plan(fimex_amd_vector_plan& plan, const double* h_matrix);
void launch_vector_values(const fimex_amd_vector_plan& plan, float* d_u, float* d_v, size_t oz, hipStream_t stream);
void launch_vector_direction_scaled(const fimex_amd_vector_plan& plan, float* d_angles, size_t oz, double scale, double offset, hipStream_t stream);
void launch_vector_direction(const fimex_amd_vector_plan& plan, float* d_angles, size_t oz, hipStream_t stream);

// convert.hip
void launch_bad2nan(float* d, size_t n, float bad, hipStream_t stream);
void launch_nan2bad(float* d, size_t n, float bad, hipStream_t stream);
void launch_points2position(double* d_points, size_t n, const double* h_axis, int num, int axisType, hipStream_t stream);
bool launch_get_values_1d_f(int kind, const float* A, const float* B, float* out, size_t n, double a, double b, double x, hipStream_t stream);
void launch_get_values_linear_d(const double* A, const double* B, double* out, size_t n, double a, double b, double x, hipStream_t stream);
size_t cdm_type_size(int cdmType);  // throws for types without a float form
void launch_data2interpolation(const void* d_in, int cdmType, size_t n, double badValue, float* d_out, hipStream_t stream);
void launch_interpolation2data(const float* d_in, size_t n, int cdmType, double badValue, void* d_out, hipStream_t stream);

// f(T{}) with the C++ type of a numeric fimex_amd_datatype (char is signed on the reference's platforms); throws as cdm_type_size
template <class F>
void for_cdm_type(int cdmType, F&& f)
{
    switch (cdmType) {
    case FIMEX_AMD_CDM_CHAR: f((signed char)0); break;
    case FIMEX_AMD_CDM_SHORT: f((short)0); break;
    case FIMEX_AMD_CDM_INT: f((int)0); break;
    case FIMEX_AMD_CDM_FLOAT: f((float)0); break;
    case FIMEX_AMD_CDM_DOUBLE: f((double)0); break;
    case FIMEX_AMD_CDM_UCHAR: f((unsigned char)0); break;
    case FIMEX_AMD_CDM_USHORT: f((unsigned short)0); break;
    case FIMEX_AMD_CDM_UINT: f((unsigned int)0); break;
    case FIMEX_AMD_CDM_INT64: f((long long)0); break;
    case FIMEX_AMD_CDM_UINT64: f((unsigned long long)0); break;
    default: (void)cdm_type_size(cdmType);
    }
}

// scaled_convert.hip: ScaleValue<IN, OUT> between stored types
bool scaled_fill_representable(int cdmType, double fill);  // static_cast<T>(fill) is defined
void launch_convert_scaled(const void* d_in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType, double newFill,
                           double newScale, double newOffset, void* d_out, hipStream_t stream);

// pressure_convert.hip: theta2T and specific2relative of CDMPressureConversions on a level description
void launch_theta_to_temperature(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_theta, float addOffset,
                                 float* d_T, hipStream_t stream);
void launch_specific_to_relative_humidity(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_q,
                                          const float* d_T, short* d_rh, hipStream_t stream);

// time_accumulate.hip: accumulate / deAccumulate of CDMProcessor along the unlimited dimension
void launch_accumulate(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* d_prev, double* d_out, hipStream_t stream);
void launch_deaccumulate(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* d_prev, double* d_out,
                         hipStream_t stream);

// time_interpolate.hip: a series onto a new time axis (CDMTimeInterpolator); one entry per output step, worked out on the host
using TimeStepClass = blend_math::Class;  // of linear_weak_extrapol: CopyA, CopyB, Blend or Undefined
struct TimeStep {
    uint32_t t1, t2;  // the pair of input slices
    float f;          // the blend factor of interpolation.c:1087
    TimeStepClass cls;
};
void launch_time_interpolate(const void* d_in, int cdmType, size_t n, const TimeStep* h_steps, size_t nNew, float* d_out, hipStream_t stream);

// quality.hip: the status rules of CDMQualityExtractor, in place on the data
struct QualityRule {
    int mode;  // fimex_amd_quality_mode
    double limit, validMin, validMax, statusFill;
    const double* h_values;  // VALUES: sorted, without NaN
    size_t nValues;
};
bool quality_mode_known(int mode);
bool quality_fill_representable(int cdmType, double fill);  // data_caster<C, double>(fill) gives the rounded fill back
void launch_quality_mask(void* d_data, int dataType, size_t nData, const void* d_status, int statusType, size_t nStatus, const QualityRule& rule,
                         double fillValue, hipStream_t stream);

// vertical.hip: vertical interpolation to fixed or template levels
bool vertical_method_known(int method);
void check_vertical_levels(const fimex_amd_vertical_levels* levels, const char* which, bool nonEmpty);  // throws: unknown kind, missing array
// what the one-shot entries and the plan's create refuse alike; false: emptyIsDone and no cells, nothing has been asked beyond the levels
bool check_vertical_search(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                           const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, bool emptyIsDone);
void launch_vertical_interpolate(int method, size_t nx, size_t ny, size_t nt, const float* d_in, const fimex_amd_vertical_levels& inLevels,
                                 const fimex_amd_vertical_levels* outLevels, const double* h_level1, size_t nzo, const double* d_validMin,
                                 const double* d_validMax, float clampMin, float clampMax, float* d_out, hipStream_t stream);
void launch_vertical_levels(const fimex_amd_vertical_levels& levels, size_t nx, size_t ny, size_t nt, float* d_out, hipStream_t stream);

// vertical_levels.hip: the level converters for altitude, height and ocean depth
bool vertical_order_known(int surfaceFirst);
void launch_vertical_altitude(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_T, const float* d_q,
                              const float* d_sap, const float* d_sgp, int surfaceFirst, const double* d_topo, double topoFactor, float* d_out,
                              hipStream_t stream);
void launch_vertical_standard(bool toPressure, const fimex_amd_vertical_levels& levels, size_t nx, size_t ny, size_t nt, const double* d_topo,
                              double topoFactor, float* d_out, hipStream_t stream);
void launch_vertical_ocean_depth(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* h_s, const double* h_C, double depth_c,
                                 const double* d_depth, const double* d_eta, float* d_out, hipStream_t stream);

// vertical_velocity.hip: grid distances, the vertical velocity on model levels, omega to vertical wind
void launch_griddistance(size_t nx, size_t ny, const double* d_lon, const double* d_lat, float* d_distX, float* d_distY, hipStream_t stream);
void launch_vertical_velocity(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* d_distX, const float* d_distY,
                              const double* h_ap, const double* h_b, const float* d_zs, const float* d_ps, const float* d_u, const float* d_v,
                              const float* d_t, float* d_w, hipStream_t stream);
void launch_omega_to_vertical_wind(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_omega,
                                   const float* d_t, float* d_w, hipStream_t stream);

// merge.hip: border smoothing, overlay, and CDMMerger's four steps fused or as a chain of the existing applies
void launch_border_smooth(const float* d_inner, const float* d_outerOnInner, float* d_out, size_t nx, size_t ny, size_t nz, size_t transitionWidth,
                          size_t borderWidth, bool useOuter, hipStream_t stream);
void launch_overlay(const float* d_top, const float* d_base, float* d_out, size_t n, hipStream_t stream);
void launch_merge_fused(const fimex_amd_merge_plan& m, const float* d_inner, const float* d_outer, size_t nz, float* d_out, hipStream_t stream);
void launch_merge_chain(const fimex_amd_merge_plan& m, const float* d_inner, const float* d_outer, size_t nz, float* d_out, hipStream_t stream);

// merge_typed.hip: the same on variables in their stored types, each with its own packing; the result has the inner's.
// launch_merge_typed_fused returns false, with nothing launched, where the fused kernels do not serve the call
void launch_border_smooth_typed(const void* d_inner, const fimex_amd_packing& pi, const void* d_outerOnInner, const fimex_amd_packing& po, void* d_out,
                                size_t nx, size_t ny, size_t nz, size_t transitionWidth, size_t borderWidth, bool useOuter, hipStream_t stream);
void launch_overlay_typed(const void* d_top, const fimex_amd_packing& pt, const void* d_base, const fimex_amd_packing& pb, void* d_out, size_t n,
                          hipStream_t stream);
bool launch_merge_typed_fused(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer,
                              const fimex_amd_packing& po, size_t nz, void* d_out, hipStream_t stream);
void launch_merge_typed_chain(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer,
                              const fimex_amd_packing& po, size_t nz, void* d_out, hipStream_t stream);

// merge_vector.hip: the same on an x/y vector pair of float arrays, rotated behind each of the three regrids
void launch_merge_vector_fused(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                               const fimex_amd_vector_plan& rotOT, const float* d_innerU, const float* d_innerV, const float* d_outerU,
                               const float* d_outerV, size_t nz, float* d_outU, float* d_outV, hipStream_t stream);
void launch_merge_vector_chain(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                               const fimex_amd_vector_plan& rotOT, const float* d_innerU, const float* d_innerV, const float* d_outerU,
                               const float* d_outerV, size_t nz, float* d_outU, float* d_outV, hipStream_t stream);

// merge_vector_typed.hip: the same on an x/y vector pair in its stored types; every one of the four fields has its own packing,
// outU has inner u's, outV inner v's.  launch_merge_vector_typed_fused returns false, with nothing launched, where the fused
// kernels do not serve the call
struct PackedVectorFields {
    const void *d_innerU, *d_innerV, *d_outerU, *d_outerV;
    fimex_amd_packing innerUPacking, innerVPacking, outerUPacking, outerVPacking;
};
bool launch_merge_vector_typed_fused(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                                     const fimex_amd_vector_plan& rotOT, const PackedVectorFields& in, size_t nz, void* d_outU, void* d_outV,
                                     hipStream_t stream);
void launch_merge_vector_typed_chain(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                                     const fimex_amd_vector_plan& rotOT, const PackedVectorFields& in, size_t nz, void* d_outU, void* d_outV,
                                     hipStream_t stream);

// projection.hip: pj_transform-level plan building on the device (strings: projection_parse.hip, point math: proj_math.hpp)
void launch_project_values(const char* projIn, const char* projOut, double* d_x, double* d_y, size_t n, hipStream_t stream);
void launch_project_axes(const char* projIn, const char* projOut, const double* h_xAxis, const double* h_yAxis, size_t ix, size_t iy,
                         double* d_outX, double* d_outY, hipStream_t stream);
void launch_vector_reproject_matrix(const char* projIn, const char* projOut, const double* h_outXAxis, const double* h_outYAxis,
                                    int xAxisType, int yAxisType, size_t ox, size_t oy, double* d_matrix, hipStream_t stream);
void launch_vector_reproject_matrix_field(const char* projIn, const char* projOut, const double* h_inX, const double* h_inY, size_t ox,
                                          size_t oy, double* d_matrix, hipStream_t stream);
void launch_vector_reproject_matrix_points(const char* projIn, const char* projOut, int inputIsMetric, const double* h_outX,
                                           const double* h_outY, size_t on, double* d_matrix, hipStream_t stream);
int projection_is_degree(const char* proj);

// coordsearch.hip: coordinate-based nearest neighbour plans
double grid_distance(const double* d_lon, const double* d_lat, size_t orgX, size_t orgY, hipStream_t stream);
void launch_coord_nearest(double* d_pointsX, double* d_pointsY, size_t nPoints, const double* d_lon, const double* d_lat, size_t orgX,
                          size_t orgY, hipStream_t stream);
void launch_coord_kdtree(double maxDist, double* d_pointsX, double* d_pointsY, size_t nPoints, const double* d_lon, const double* d_lat,
                         size_t orgX, size_t orgY, hipStream_t stream);

// fill_rects.hip (the fills, whole or by rectangles) and fill_sum.hip (run_scan_sum)
void run_fill2d(size_t nx, size_t ny, size_t nz, float* d_field, float relaxCrit, float corrEff, size_t maxLoop,
                size_t* h_nChanged, hipStream_t stream);
void run_creepfill(size_t nx, size_t ny, size_t nz, float* d_field, bool useDefault, float defaultVal,
                   unsigned short repeat, char setWeight, size_t* h_nChanged, hipStream_t stream);

void run_scan_sum(const float* d_values, size_t n, int mode, double average, int algo, double* h_sum, size_t* h_nUndefined,
                  hipStream_t stream);

// batch.hip: output batches placed by the library
fimex_amd_batch* batch_alloc(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, int positions, hipStream_t stream);
fimex_amd_batch* batch_alloc_source(const fimex_amd_regrid_plan& plan, size_t nz, int candidates, hipStream_t stream);
void batch_free(fimex_amd_batch* batch);
const fimex_amd_batch_info& batch_info(const fimex_amd_batch& batch);
void apply_plan_device(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream);
void apply_plan_typed_device(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                             hipStream_t stream);
// capi_vector.hip: a vector pair regridded and rotated as fimex_amd_regrid_apply_vector_device serves it; returns the path taken
int apply_vector_pair(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const float* d_u, const float* d_v, size_t nz,
                      float* d_uOut, float* d_vOut, hipStream_t stream);
// the same on the components' stored types as fimex_amd_regrid_apply_vector_typed_device serves it (the chain of
// merge_vector_typed.hip runs it too)
int apply_vector_pair_typed(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const void* d_u, int uType, double uBad,
                            const void* d_v, int vType, double vBad, size_t nz, void* d_uOut, void* d_vOut, hipStream_t stream);

// hostpipe.hip: streamed transfers for the *_host entry points
using SliceChunkFn = std::function<void(const void* dRawIn, void* dRawOut, float* dFIn, float* dFOut, size_t nzc, hipStream_t stream)>;
bool pipelined_slices(int device, const void* in, size_t inSliceBytes, void* out, size_t outSliceBytes, size_t inSliceFloats,
                      size_t outSliceFloats, size_t nz, const SliceChunkFn& fn);

void host_to_device(void* d_dst, const void* h_src, size_t bytes, hipStream_t stream);
void device_to_host(void* h_dst, const void* d_src, size_t bytes, hipStream_t stream);
void release_host_pipes();

// experiment switches: the measured default in the product library; the tuning build (-DFIMEX_AMD_TUNING) reads FIMEX_AMD_<NAME>
// from the environment at every call, so that one process can sweep settings (capi.hip)
int tuning(const char* name, int fallback);

// slices per z chunk of the second form's float launches in tile-major and chunk-per-XCD order (staged2_z_chunks, staged2.hpp, and
// fimex_amd_regrid_plan_tune_device share it)
inline uint32_t staged2_zpb() { return (uint32_t)tuning("STAGE2_ZPB", 25); }

}  // namespace fimex_amd
