// The reference's backward stencil rules, stated once: which source cells an output cell reads, how a plan entry says so,
// and the arithmetic of mifi_get_values_f / _bilinear_f / _bicubic_f (src/interpolation.c:862-1028) operation by operation.
// Every backward kernel (backward_plan.hip, gather.hip, merge.hip, staged.hip, staged2.hip) takes them from here, and so does the host shim of
// tests/test_stencil_math_host.py, which checks this file against the reference's arithmetic on the CPU, without a GPU:
// everything is __host__ __device__ and free of device builtins.  Compiled with -ffp-contract=off: every multiply and add is a separate
// IEEE operation in the reference's type and order.
#pragma once

#include "plan.hpp"

#include <cmath>
#include <type_traits>

#define FA_HD __host__ __device__ __forceinline__

namespace fimex_amd {

// coordinates beyond this, NaN or inf are "outside" (the reference casts them to int: undefined behaviour)
FA_HD bool usable(double x, double y)
{
    const double lim = 1073741824.0;
    return (fabs(x) < lim) && (fabs(y) < lim);  // false for NaN
}

// which source cells one output cell reads: columns xa..xb of rows ya..yb (inclusive)
struct CellNeed {
    bool valid;
    int64_t xa, xb, ya, yb;
};

// STENCIL 1: nearest (src/interpolation.c:862-879); 2: bilinear incl. its border branches (:883-954); 4: bicubic (:970-976)
template <int STENCIL>
FA_HD CellNeed classify(double x, double y, int64_t ix, int64_t iy)
{
    CellNeed c{};
    c.valid = false;
    if (!usable(x, y)) return c;
    if (STENCIL == 1) {  // nearest: lround half away from zero (:864-868)
        const int64_t rx = (int64_t)round(x), ry = (int64_t)round(y);
        if (rx >= 0 && rx < ix && ry >= 0 && ry < iy) { c.valid = true; c.xa = c.xb = rx; c.ya = c.yb = ry; }
        return c;
    }
    const int64_t x0 = (int64_t)floor(x), y0 = (int64_t)floor(y);
    if (STENCIL == 4) {
        if ((1 <= x0) && (x0 + 2 < ix) && (1 <= y0) && (y0 + 2 < iy)) {
            c.valid = true; c.xa = x0 - 1; c.xb = x0 + 2; c.ya = y0 - 1; c.yb = y0 + 2;
        }
        return c;
    }
    const bool xlin = (0 <= x0) && (x0 + 1 < ix);
    const bool ylin = (0 <= y0) && (y0 + 1 < iy);
    if (xlin && ylin) {
        c.valid = true; c.xa = x0; c.xb = x0 + 1; c.ya = y0; c.yb = y0 + 1;
    } else if (xlin) {
        const int64_t ry = (int64_t)round(y);  // :904
        if (0 <= ry && ry < iy) { c.valid = true; c.xa = x0; c.xb = x0 + 1; c.ya = c.yb = ry; }
    } else {
        const int64_t rx = (int64_t)round(x);  // :922
        if (0 <= rx && rx < ix) {
            if (ylin) {
                c.valid = true; c.xa = c.xb = rx; c.ya = y0; c.yb = y0 + 1;
            } else {
                const int64_t ry = (int64_t)round(y);  // :935
                // the reference tests "ry <= iy" (:936) and then reads past the slice; undefined here
                if (0 <= ry && ry < iy) { c.valid = true; c.xa = c.xb = rx; c.ya = c.yb = ry; }
            }
        }
    }
    return c;
}

// ---- plan entries (plan.hpp).  pos is the first cell of the stencil, kInvalidPos for an undefined output.  Bilinear: xf / yf
// are the fractions rounded to float as :885,888 do; a set sign bit (-1.f) says "one column" / "one row" -- the border
// branches :903-948, pos then points at the rounded cell.  Bicubic: the double fractions of :971,973.  The fractions of an
// undefined output are 0.
FA_HD uint32_t encode_pos(const CellNeed& c, int64_t ix)
{
    return c.valid ? (uint32_t)(c.ya * ix + c.xa) : kInvalidPos;
}
FA_HD float encode_frac_bilinear(const CellNeed& c, bool one, double v)
{
    if (!c.valid) return 0.f;
    return one ? -1.f : (float)(v - floor(v));  // double difference rounded to float
}
FA_HD double encode_frac_bicubic(const CellNeed& c, double v) { return c.valid ? v - floor(v) : 0.; }

FA_HD bool is_nn(float frac) { return (__builtin_bit_cast(uint32_t, frac) >> 31) != 0; }
// the same as a selection mask: all ones for "nearest neighbour in this direction"
FA_HD uint32_t nn_mask(float frac) { return (uint32_t)(__builtin_bit_cast(int32_t, frac) >> 31); }

// the cells a plan entry stands for: what classify<STENCIL> said when the entry was written
template <int STENCIL>
FA_HD CellNeed entry_need(uint32_t pos, float xf, float yf, int64_t ix)
{
    CellNeed c{};
    c.valid = pos != kInvalidPos;
    if (!c.valid) return c;
    c.ya = (int64_t)(pos / (uint32_t)ix);
    c.xa = (int64_t)pos - c.ya * ix;
    if (STENCIL == 1) { c.xb = c.xa; c.yb = c.ya; }
    else if (STENCIL == 2) { c.xb = c.xa + (is_nn(xf) ? 0 : 1); c.yb = c.ya + (is_nn(yf) ? 0 : 1); }
    else { c.xb = c.xa + 3; c.yb = c.ya + 3; }
    return c;
}

// ---- bilinear (:883-954).  s00 is the cell at pos, s01 its right neighbour, s10 / s11 the row below.
struct BilinearForms {
    float top;    // linear in x on the upper row: the value when nearest in y (:911)
    float inter;  // interior cell (:899-900)
    float liny;   // nearest in x, linear in y (:931)
};
FA_HD BilinearForms bilinear_forms(float s00, float s01, float s10, float s11, float xf, float yf)
{
    BilinearForms f;
    f.top = (1.f - xf) * s00 + xf * s01;
    const float bot = (1.f - xf) * s10 + xf * s11;
    f.inter = (1.f - yf) * f.top + yf * bot;
    f.liny = (1 - yf) * s00 + (yf * s10);
    return f;
}
// nearest in both directions: the cell itself (:939-942)
FA_HD float bilinear_select(BilinearForms f, float s00, bool nnx, bool nny)
{
    return nnx ? (nny ? s00 : f.liny) : (nny ? f.top : f.inter);
}
// Every form evaluated, one selected: no lane leaves the common path.  A border entry never selects a form that reads the
// cells it lacks, so the caller may pass anything for them (the kernels repeat s00).
FA_HD float bilinear_value(float s00, float s01, float s10, float s11, float xf, float yf)
{
    return bilinear_select(bilinear_forms(s00, s01, s10, s11, xf, yf), s00, is_nn(xf), is_nn(yf));
}

// ---- bicubic (:956-1028).  Keys kernel a = -0.5: rows of M/2 (:962-968), weights XM / MY (:977-1000)
FA_HD void cubic_weights(double f, double w[4])
{
    const double M[4][4] = {{0.0, 1.0, 0.0, 0.0}, {-0.5, 0.0, 0.5, 0.0}, {1.0, -2.5, 2.0, -0.5}, {-0.5, 1.5, -1.5, 0.5}};
    double X[4];
    X[0] = 1;
    X[1] = f;
    X[2] = f * f;
    X[3] = X[2] * f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += X[j] * M[j][i];
        w[i] = s;
    }
}

// one 4x4 stencil, f[row][column]: XMF[i] = sum_j XM[j] * F[j][i] (:1015), out += XMF[i] * MY[i] into the float (:1005,1019)
FA_HD float bicubic_point(const float f[4][4], const double XM[4], const double MY[4])
{
    float acc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double xmf = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) xmf += XM[j] * (double)f[i][j];
        acc = (float)((double)acc + xmf * MY[i]);
    }
    return acc;
}

// ---- one plan entry, decoded: the step from (pos, fractions) to a value that every gather kernel (gather_entry.hpp), the merger and
// the host shim take.  first: the stencil's first cell; dx / dy: the steps in cells to its next column / row, 0 for a neighbour
// the entry lacks (bilinear border entries) and for an undefined entry, whose taps then all name one cell.
template <int STENCIL>
using frac_t = typename std::conditional<STENCIL == 4, double, float>::type;  // xf / yf, or xfd / yfd (nearest: none, pass 0)

template <int STENCIL>
struct EntryWeights {};
template <>
struct EntryWeights<2> {
    float xf, yf;
};
template <>
struct EntryWeights<4> {
    double XM[4], MY[4];
};

template <int STENCIL>
struct StencilEntry : EntryWeights<STENCIL> {
    bool valid;
    uint32_t first, dx, dy;

    // taps[row][column]: the tap itself, bilinear_value (every form evaluated, one selected) or bicubic_point
    FA_HD float combine(const float (&taps)[STENCIL][STENCIL]) const
    {
        if constexpr (STENCIL == 2) return bilinear_value(taps[0][0], taps[0][1], taps[1][0], taps[1][1], this->xf, this->yf);
        else if constexpr (STENCIL == 4) return bicubic_point(taps, this->XM, this->MY);
        else return taps[0][0];
    }
};

template <int STENCIL>
FA_HD StencilEntry<STENCIL> decode_entry(uint32_t pos, frac_t<STENCIL> xf, frac_t<STENCIL> yf, uint32_t ix)
{
    StencilEntry<STENCIL> e;
    e.valid = pos != kInvalidPos;
    e.first = pos;
    e.dx = (e.valid && STENCIL != 1) ? 1u : 0u;
    e.dy = (e.valid && STENCIL != 1) ? ix : 0u;
    if constexpr (STENCIL == 2) {
        e.xf = xf;
        e.yf = yf;
        if (is_nn(xf)) e.dx = 0u;
        if (is_nn(yf)) e.dy = 0u;
    } else if constexpr (STENCIL == 4) {
        cubic_weights(xf, e.XM);
        cubic_weights(yf, e.MY);
    }
    return e;
}

}  // namespace fimex_amd
