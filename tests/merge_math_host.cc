// fimex_amd/csrc/merge_math.hpp compiled for the CPU with a plain C++ compiler (fimex_amd/build.py: build_merge_math_host), used
// the way merge_typed.hip uses it: a class per cell, the typed cell functions on every slice.  tests/test_merge_math_host.py
// compares the results with the restatement of tests/merge_typed_ref.py byte for byte.
#include "merge_math.hpp"

#include <cstddef>

namespace mm = fimex_amd::merge_math;

namespace {

struct PackingArg {
    int type;
    double fill, scale, offset;
};

// f(T{}) with the C++ type of a numeric CDMDataType code; false for every other code
template <class F>
bool for_type(int code, F&& f)
{
    switch (code) {
    case 1: f((signed char)0); return true;
    case 2: f((short)0); return true;
    case 3: f((int)0); return true;
    case 4: f((float)0); return true;
    case 5: f((double)0); return true;
    case 7: f((unsigned char)0); return true;
    case 8: f((unsigned short)0); return true;
    case 9: f((unsigned int)0); return true;
    case 10: f((long long)0); return true;
    case 11: f((unsigned long long)0); return true;
    default: return false;
    }
}

}  // namespace

extern "C" {

// the float form, as merge.hip's kernels use it
int merge_math_smooth_float(const float* inner, const float* outer, float* out, size_t nx, size_t ny, size_t nz, size_t tw, size_t bw, int useOuter)
{
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            const mm::SmoothClass c = mm::smooth_class(x, y, nx, ny, tw, bw);
            for (size_t z = 0; z < nz; ++z) {
                const size_t i = (z * ny + y) * nx + x;
                out[i] = mm::smooth_value<float>(c, inner[i], mm::needs_outer<float>(c, inner[i], useOuter != 0) ? outer[i] : 0.f, useOuter != 0);
            }
        }
    return 0;
}

int merge_math_smooth_typed(const void* inner, const PackingArg* pi, const void* outer, const PackingArg* po, void* out, size_t nx, size_t ny, size_t nz,
                            size_t tw, size_t bw, int useOuter)
{
    bool ran = false;
    for_type(pi->type, [&](auto ti) {
        for_type(po->type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            if (!mm::representable<TI>(pi->fill)) return;
            const mm::Unpack<TI> unI = mm::make_unpack<TI>(pi->fill, pi->scale, pi->offset);
            const mm::Unpack<TO> unO = mm::make_unpack<TO>(po->fill, po->scale, po->offset);
            const mm::Pack<TI> pack = mm::make_pack<TI>(pi->fill, pi->scale, pi->offset);
            const TI* I = static_cast<const TI*>(inner);
            const TO* O = static_cast<const TO*>(outer);
            TI* S = static_cast<TI*>(out);
            for (size_t y = 0; y < ny; ++y)
                for (size_t x = 0; x < nx; ++x) {
                    const mm::SmoothClass c = mm::smooth_class(x, y, nx, ny, tw, bw);
                    for (size_t z = 0; z < nz; ++z) {
                        const size_t i = (z * ny + y) * nx + x;
                        S[i] = mm::smooth_cell_typed<TI, TO>(c, I[i], O[i], unI, unO, pack, useOuter != 0);
                    }
                }
            ran = true;
        });
    });
    return ran ? 0 : -1;
}

int merge_math_overlay_typed(const void* top, const PackingArg* pt, const void* base, const PackingArg* pb, void* out, size_t n)
{
    bool ran = false;
    for_type(pt->type, [&](auto ti) {
        for_type(pb->type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            if (!mm::representable<TI>(pt->fill)) return;
            const mm::Unpack<TI> unI = mm::make_unpack<TI>(pt->fill, pt->scale, pt->offset);
            const mm::Unpack<TO> unO = mm::make_unpack<TO>(pb->fill, pb->scale, pb->offset);
            const mm::Pack<TI> pack = mm::make_pack<TI>(pt->fill, pt->scale, pt->offset);
            for (size_t i = 0; i < n; ++i)
                static_cast<TI*>(out)[i] = mm::overlay_cell_typed<TI, TO>(static_cast<const TI*>(top)[i], static_cast<const TO*>(base)[i], unI, unO, pack);
            ran = true;
        });
    });
    return ran ? 0 : -1;
}

// steps 3 and 4 from the two regrids' float results; both fill values must be representable in their types
int merge_math_regrid_overlay_typed(const float* top, const PackingArg* pt, const float* base, const PackingArg* pb, void* out, size_t n)
{
    bool ran = false;
    for_type(pt->type, [&](auto ti) {
        for_type(pb->type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            if (!mm::representable<TI>(pt->fill) || !mm::representable<TO>(pb->fill)) return;
            const mm::Unpack<TI> unI = mm::make_unpack<TI>(pt->fill, pt->scale, pt->offset);
            const mm::Unpack<TO> unO = mm::make_unpack<TO>(pb->fill, pb->scale, pb->offset);
            const mm::Pack<TI> pack = mm::make_pack<TI>(pt->fill, pt->scale, pt->offset);
            const TI fillI = static_cast<TI>(pt->fill);
            const TO fillO = static_cast<TO>(pb->fill);
            for (size_t i = 0; i < n; ++i) {
                const bool need = mm::overlay_needs_base<TI>(mm::round_to_stored<TI>(top[i], fillI), unI);
                static_cast<TI*>(out)[i] = mm::regrid_overlay_cell_typed<TI, TO>(top[i], fillI, need ? base[i] : 0.f, fillO, unI, unO, pack);
            }
            ran = true;
        });
    });
    return ran ? 0 : -1;
}

}  // extern "C"
