// Host-side geometry of the fills by rectangles (fill_rects.hip, run_creepfill and run_fill2d): pure C++, no device code --
// tests/test_creep_rects.py compiles it on its own and checks its invariants on random masks.  Line numbers such as :1266-1269 are
// those of the reference's src/interpolation.c.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace fimex_amd {
namespace creep_rects {

struct Rect {
    uint32_t xa, xb, ya, yb;  // inclusive, ring included
    bool operator==(const Rect& o) const { return xa == o.xa && xb == o.xb && ya == o.ya && yb == o.yb; }
};

// maximal runs of set flags -> intervals with one clean element on either side (or the array's end), at least minLen long where
// the array allows, merged where they overlap by more than a shared boundary
inline std::vector<std::pair<uint32_t, uint32_t>> dirty_intervals(const std::vector<unsigned char>& dirty, uint32_t minLen)
{
    const uint32_t n = (uint32_t)dirty.size();
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (uint32_t i = 0; i < n;) {
        if (!dirty[i]) { ++i; continue; }
        uint32_t j = i;
        while (j + 1 < n && dirty[j + 1]) ++j;
        uint32_t a = i > 0 ? i - 1 : 0, b = j + 1 < n ? j + 1 : n - 1;
        while (b - a + 1 < minLen && (b + 1 < n || a > 0)) {  // grow over clean elements (a later dirty one: merged below)
            if (b + 1 < n) ++b;
            else --a;
        }
        out.emplace_back(a, b);
        i = j + 1;
    }
    // merge: an interval that reaches into the next one's dirty elements
    std::vector<std::pair<uint32_t, uint32_t>> merged;
    for (const auto& iv : out) {
        if (!merged.empty() && iv.first < merged.back().second) merged.back().second = std::max(merged.back().second, iv.second);
        else merged.push_back(iv);
    }
    // the ends must be clean or the array's ends: growing may have stopped on a dirty element of a neighbour that was merged away
    for (auto& iv : merged) {
        while (iv.first > 0 && dirty[iv.first]) --iv.first;
        while (iv.second + 1 < n && dirty[iv.second]) ++iv.second;
    }
    std::vector<std::pair<uint32_t, uint32_t>> fin;
    for (const auto& iv : merged) {
        if (!fin.empty() && iv.first < fin.back().second) fin.back().second = std::max(fin.back().second, iv.second);
        else fin.push_back(iv);
    }
    return fin;
}

// Undefined cells inside rectangle r (whose ring is defined, or the field's border) -> the rectangles that hold them: runs of rows
// with undefined cells x runs of columns with undefined cells in those rows, each looked at again on its own (the rows a column
// run needs are often fewer than the row run it came from).
inline void refine_rect(const uint32_t* bits, uint32_t words, const Rect& r, int depth, std::vector<Rect>& out)
{
    const uint32_t w = r.xb - r.xa + 1, h = r.yb - r.ya + 1;
    const uint32_t k0 = r.xa >> 5, k1 = r.xb >> 5;
    auto word_mask = [&](uint32_t k) -> uint32_t {
        uint32_t m = 0xFFFFFFFFu;
        if (k == k0) m &= 0xFFFFFFFFu << (r.xa & 31);
        if (k == k1) m &= 0xFFFFFFFFu >> (31 - (r.xb & 31));
        return m;
    };
    std::vector<unsigned char> rowDirty(h, 0);
    for (uint32_t y = 0; y < h; ++y) {
        uint32_t any = 0;
        for (uint32_t k = k0; k <= k1; ++k) any |= bits[(size_t)(r.ya + y) * words + k] & word_mask(k);
        rowDirty[y] = any != 0;
    }
    for (const auto& rv : dirty_intervals(rowDirty, 4)) {
        std::vector<uint32_t> orw(k1 - k0 + 1, 0);
        for (uint32_t y = rv.first; y <= rv.second; ++y)
            for (uint32_t k = k0; k <= k1; ++k) orw[k - k0] |= bits[(size_t)(r.ya + y) * words + k] & word_mask(k);
        std::vector<unsigned char> colDirty(w, 0);
        for (uint32_t x = 0; x < w; ++x) { const uint32_t ax = r.xa + x; colDirty[x] = (orw[(ax >> 5) - k0] >> (ax & 31)) & 1u; }
        for (const auto& cv : dirty_intervals(colDirty, 4)) {
            const Rect q{r.xa + cv.first, r.xa + cv.second, r.ya + rv.first, r.ya + rv.second};
            if (q == r || depth == 0) out.push_back(q);
            else refine_rect(bits, words, q, depth - 1, out);
        }
    }
}

// the rectangles of one slice from its NaN bitmap; false: not worth it, take the whole slice
inline bool slice_rects(const uint32_t* bits, uint32_t nx, uint32_t ny, uint32_t words, std::vector<Rect>& rects)
{
    rects.clear();
    refine_rect(bits, words, Rect{0, nx - 1, 0, ny - 1}, 4, rects);
    size_t area = 0;
    for (const Rect& r : rects) area += (size_t)(r.xb - r.xa + 1) * (r.yb - r.ya + 1);
    return !rects.empty() && rects.size() <= 64 && area * 2 <= (size_t)nx * ny;
}

// ---- what the drivers in fill_rects.hip do with the rectangles

// Is the slice with these undefined cells per row (and, fill2d, defined cells that hold -0.0 or an infinity: `special`, may be
// null) a candidate?  0: nothing to fill or nothing defined, the slice is left alone (:1266-1269, :1384-1386); -1: holes scattered
// over (nearly) all rows leave nothing to cut, or a special cell forbids it; 1: look for rectangles
inline int slice_candidate(const uint32_t* rowCount, const uint32_t* special, size_t ny, size_t total)
{
    size_t dirtyRows = 0, undefined = 0, specials = 0;
    for (size_t y = 0; y < ny; ++y) {
        dirtyRows += rowCount[y] != 0;
        undefined += rowCount[y];
        if (special) specials += special[y];
    }
    if (undefined == 0 || undefined == total) return 0;
    return (dirtyRows * 10 > ny * 9 || specials != 0) ? -1 : 1;
}

// fill2d pads the rectangles of a slice to one box size
inline void box_size(const std::vector<Rect>& rects, size_t& mw, size_t& mh)
{
    mw = mh = 0;
    for (const Rect& r : rects) { mw = std::max<size_t>(mw, r.xb - r.xa + 1); mh = std::max<size_t>(mh, r.yb - r.ya + 1); }
}
// ... which is worth it while the boxes cover at most half of the slice
inline bool padded_boxes_worth_it(const std::vector<Rect>& rects, size_t total)
{
    size_t mw, mh;
    box_size(rects, mw, mh);
    return rects.size() * mw * mh * 2 <= total;
}
// where rectangle q sits in its box of mw x mh cells: a side on the field's far border stays on the box's border (its cells are
// the ones :1363-1370 work on); one that spans the field has both borders on the box's, being as wide as box_size's box
inline std::pair<uint32_t, uint32_t> box_offset(const Rect& q, size_t nx, size_t ny, size_t mw, size_t mh)
{
    const size_t w = q.xb - q.xa + 1, h = q.yb - q.ya + 1;
    return {(q.xb == nx - 1 && q.xa != 0) ? (uint32_t)(mw - w) : 0u, (q.yb == ny - 1 && q.ya != 0) ? (uint32_t)(mh - h) : 0u};
}
// end (exclusive) of the run of consecutive slices from z0 with the same rectangles and the same `skip`, at most `most` slices
// (masks usually do not change from slice to slice)
inline size_t same_rects_run(const std::vector<std::vector<Rect>>& rects, const std::vector<unsigned char>& skip, size_t z0, size_t most)
{
    size_t z1 = z0 + 1;
    while (z1 < rects.size() && z1 - z0 < most && rects[z1] == rects[z0] && skip[z1] == skip[z0]) ++z1;
    return z1;
}
// the rectangles grouped by size, groups in the order of their first member, members in their own order
inline std::vector<std::vector<Rect>> rects_by_size(const std::vector<Rect>& rects)
{
    std::vector<std::vector<Rect>> groups;
    std::vector<char> done(rects.size(), 0);
    for (size_t i = 0; i < rects.size(); ++i) {
        if (done[i]) continue;
        const uint32_t w = rects[i].xb - rects[i].xa, h = rects[i].yb - rects[i].ya;
        groups.emplace_back();
        for (size_t j = i; j < rects.size(); ++j)
            if (!done[j] && rects[j].xb - rects[j].xa == w && rects[j].yb - rects[j].ya == h) { groups.back().push_back(rects[j]); done[j] = 1; }
    }
    return groups;
}

}  // namespace creep_rects
}  // namespace fimex_amd
