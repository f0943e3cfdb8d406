// Which kernel serves a call of the backward regrid: the one statement of the rule.  Every entry point asks here -- plan build,
// float slices, stored types, vector pairs, lists of variables -- and the launchers only check, as preconditions, what the rule
// has already decided.  Plain values in, plain values out: no HIP type, no tuning() call, no plan pointer, so that
// tests/test_backward_dispatch.py compiles it with g++ and compares every answer, over the whole cross product of its inputs,
// with the conditions the entry points used to carry themselves (tests/backward_dispatch_ref.py).
//
// Two facts stay outside, because they are only known once the launcher has looked: whether the stored-type form of the second
// staged kernel, built on first use (staged2_typed_form), exists, and whether a list kernel exists for the workgroup shape
// (list_shape).  Where they fail the caller goes on to the next candidate.
//
// Where the rules of two kernels differ without a stated reason, the difference is kept and named at its line ("differs:").
#pragma once

#include <cstdint>

#include "../../include/fimex_amd.h"

namespace fimex_amd {

enum class PlanKind { Nearest, Bilinear, Bicubic, Forward };

namespace dispatch {

// the experiment switches the rule reads; dispatch_switches() (backward_plan.hip) fills them, once per call
struct Switches {
    int staged, stagedNearest, staged2, typedFused, typedStaged, typedStaged2, vectorFused;
    uint64_t stagedMinNz;  // batches shorter than this take the gather kernels: the staged kernels pay a per-tile set-up
};

struct PlanFacts {
    PlanKind kind;
    int funcType;
    bool bicubicFast;
    bool firstValid, secondValid;  // the plan holds the first (staged.hip) / second (staged2.hip) staged form for float slices
    uint64_t inX, inY, outX, outY;
};

// one variable, a pair (cdmType2: the v component) or a list (nz: list_slices of the list, aligned: every source with slices)
struct CallFacts {
    uint64_t nz;
    int cdmType, cdmType2;
    bool aligned;  // every source pointer is 4-byte aligned (LDS-DMA pieces)
};

constexpr uint64_t kMaxSlices = 0xFFFFFFFFull;

// ---------------------------------------------------------------- plan build
inline bool builds_first(const Switches& sw, const PlanFacts& p)
{
    return sw.staged != 0 && (p.kind != PlanKind::Nearest || sw.stagedNearest != 0);
}

// The second form serves float slices, the first one stays for the stored types.  A bicubic plan in the reference's arithmetic
// keeps the first form where it exists (32 x 16 tiles at four workgroups per CU suit it) and takes the second one for the source
// widths the first cannot stage; STAGED2 = 2 prefers the second form throughout.
inline bool prefers_second(const Switches& sw, const PlanFacts& p)
{
    return sw.staged2 >= 2 || (sw.staged2 == 1 && (p.kind != PlanKind::Bicubic || !p.firstValid || p.bicubicFast));
}

// (asked after the first form has been tried: p.firstValid is its outcome)
inline bool builds_second(const Switches& sw, const PlanFacts& p) { return sw.staged != 0 && prefers_second(sw, p); }

// ---------------------------------------------------------------- float slices
enum class FloatApply : int { Second = 0, First = 1, Gather = 2 };

inline FloatApply float_apply(const Switches& sw, const PlanFacts& p, uint64_t nz)
{
    if (sw.staged == 0 || nz < sw.stagedMinNz) return FloatApply::Gather;
    if (p.secondValid && prefers_second(sw, p)) return FloatApply::Second;
    // differs: STAGED_NEAREST is not asked here (a nearest plan that holds the first form runs it), typed_first asks it
    return p.firstValid ? FloatApply::First : FloatApply::Gather;
}

// fimex_amd_regrid_plan_tune_device has something to time: a second workgroup shape, or a second launch order (secondOrder: a
// batch whose float_apply is Second and that is long enough for that order).  differs: with a second shape it asks neither
// STAGED nor STAGED2 nor which form the plan prefers, so it may time launches that do not read its choice
inline bool tune_has_choice(const Switches& sw, const PlanFacts& p, uint64_t nz, bool secondShape, bool secondOrder)
{
    return nz >= sw.stagedMinNz && p.secondValid && (secondShape || secondOrder);
}

// a list of float variables in one launch of the second form's list kernels (nz: the slices of the list together)
inline bool float_list(const Switches& sw, const PlanFacts& p, uint64_t nz) { return float_apply(sw, p, nz) == FloatApply::Second; }

// a float vector pair regridded and rotated in one launch, else the three launches it replaces (the plans of the coordinate
// searches are nearest plans too; they keep the three launches)
inline bool vector_fused(const Switches& sw, const PlanFacts& p, uint64_t nz)
{
    const bool method = p.funcType == FIMEX_AMD_INTERPOL_NEAREST_NEIGHBOR || p.funcType == FIMEX_AMD_INTERPOL_BILINEAR;
    return float_apply(sw, p, nz) == FloatApply::Second && method && sw.vectorFused != 0;
}

// ---------------------------------------------------------------- stored types
enum class TypedApply : int { Second = 0, First = 1, Gather = 2, ThreePasses = 3 };

// what the caller tries, in order; ThreePasses (to float, the float apply, from float) ends every list
struct TypedCandidates {
    int n;
    TypedApply c[4];
};

// element size of the types the staged kernels take in their stored form, 0: another type
inline uint32_t staged_elem_bytes(int cdmType)
{
    if (cdmType == FIMEX_AMD_CDM_SHORT || cdmType == FIMEX_AMD_CDM_USHORT) return 2;
    return (cdmType == FIMEX_AMD_CDM_CHAR || cdmType == FIMEX_AMD_CDM_UCHAR) ? 1u : 0u;
}

// either staged form on a stored type: the float rule's switches and batch length, 1- and 2-byte integers, slices that start on
// 4-byte boundaries
inline bool typed_staged(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    return p.kind != PlanKind::Forward && sw.typedFused != 0 && sw.staged != 0 && sw.typedStaged != 0 && c.nz >= sw.stagedMinNz &&
           staged_elem_bytes(c.cdmType) != 0 && c.aligned;
}

// differs: asks neither STAGED2 nor p.secondValid nor prefers_second -- the form is the stored type's own, built on first use
// from the gather plan, for nearest and bilinear plans; every slice must start on a 4-byte boundary
inline bool typed_second(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    return typed_staged(sw, p, c) && sw.typedStaged2 != 0 && (p.kind == PlanKind::Nearest || p.kind == PlanKind::Bilinear) &&
           (p.inX * p.inY * staged_elem_bytes(c.cdmType)) % 4 == 0;
}

inline bool typed_first(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    return typed_staged(sw, p, c) && p.firstValid && (p.kind != PlanKind::Nearest || sw.stagedNearest != 0);
}

// the gather kernel on the stored type: also int32; not bicubic (the staged float kernel between two conversion passes beats a
// 16-load gather) unless TYPED_FUSED = 2; 8 slices lie behind one 32-bit buffer descriptor.  A batch beyond kMaxSlices stays a
// candidate whatever the grid: the launcher refuses it ("too many slices"), as it did before it looked at the descriptor
inline bool typed_gather(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    const uint64_t cells = p.inX * p.inY > p.outX * p.outY ? p.inX * p.inY : p.outX * p.outY;
    return p.kind != PlanKind::Forward && sw.typedFused != 0 && (p.kind != PlanKind::Bicubic || sw.typedFused >= 2) &&
           (staged_elem_bytes(c.cdmType) != 0 || c.cdmType == FIMEX_AMD_CDM_INT) && (c.nz > kMaxSlices || 8 * 4 * cells <= 0xFFFFFFFFull);
}

inline TypedCandidates typed_apply(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    TypedCandidates t{};
    if (typed_second(sw, p, c)) t.c[t.n++] = TypedApply::Second;
    if (typed_first(sw, p, c)) t.c[t.n++] = TypedApply::First;
    if (typed_gather(sw, p, c)) t.c[t.n++] = TypedApply::Gather;
    t.c[t.n++] = TypedApply::ThreePasses;
    return t;
}

// a list of variables of one stored type in one launch of the second form's list kernel
inline bool typed_list(const Switches& sw, const PlanFacts& p, const CallFacts& c) { return typed_second(sw, p, c); }

// a vector pair on its stored type in one launch: both components short or both unsigned short, else the chain around the float
// pair.  (differs from vector_fused as typed_second differs from float_apply; batches beyond kMaxSlices take the chain, whose
// float apply refuses them)
inline bool vector_typed_fused(const Switches& sw, const PlanFacts& p, const CallFacts& c)
{
    const bool method = p.funcType == FIMEX_AMD_INTERPOL_NEAREST_NEIGHBOR || p.funcType == FIMEX_AMD_INTERPOL_BILINEAR;
    return c.cdmType == c.cdmType2 && staged_elem_bytes(c.cdmType) == 2 && typed_second(sw, p, c) && method && sw.vectorFused != 0 &&
           c.nz <= kMaxSlices;
}

}  // namespace dispatch
}  // namespace fimex_amd
