// The fills by rectangles: the entry points run_creepfill and run_fill2d.
#include "fill_prologue.hpp"
#include "creep_rects.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace fimex_amd {

namespace {

// ---- creep fill by rectangles -----------------------------------------------------------------------------------------------
// A cell that is defined on entry never changes and is read with the same weight (setWeight) whether it lies on a border or
// inside (src/interpolation.c:1408-1461).  Rows and columns that are defined throughout therefore cut the field into rectangles
// whose sweeps do not see each other, and a sweep that changes nothing ends a rectangle's loop without touching the others'
// results (further sweeps over a finished region are no-ops).  The reference sweeps the whole field until nothing changes
// anywhere: a region outside the source domain that lies ABOVE defined cells is filled one row per sweep (in-place, row-major:
// values travel down and right within a sweep, up and left one cell per sweep) -- 185 sweeps over 3000 x 3000 cells for the
// configs[4] field, of which a tenth of the field needs more than 22.  Here every rectangle (bounding box of a run of rows
// with undefined cells x a run of columns with undefined cells inside those rows, plus the defined ring around it, or the
// field's own border) is copied out, filled with the whole slice's first guess as a field of its own, and copied back.
using creep_rects::Rect;
using creep_rects::slice_rects;

// one wave per row: bit x of the row's words = cell x is undefined
// rowCount[row] = undefined cells of the row
// rowSpecial (may be null): defined cells of the row that hold -0.0 or an infinity
__global__ void __launch_bounds__(kBlock) nan_bitmap_kernel(const float* __restrict__ field, uint32_t nx, size_t rows, uint32_t words,
                                                            uint32_t* __restrict__ bits, uint32_t* __restrict__ rowCount, uint32_t* __restrict__ rowSpecial = nullptr)
{
    const size_t row = (size_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (row >= rows) return;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const float* f = field + row * nx;
    uint32_t* out = bits + row * words;
    uint32_t count = 0, special = 0;
    for (uint32_t base = 0; base < words * 32; base += kWave) {
        const uint32_t x = base + lane;
        const float v = x < nx ? f[x] : 0.f;
        const unsigned long long m = __ballot(x < nx && isnan(v));
        special += (uint32_t)__popcll(__ballot(x < nx && (__float_as_uint(v) == 0x80000000u || isinf(v))));
        count += (uint32_t)__popcll(m);
        if (lane == 0) {
            out[base / 32] = (uint32_t)m;
            if (base / 32 + 1 < words) out[base / 32 + 1] = (uint32_t)(m >> 32);
        }
    }
    if (lane == 0) {
        rowCount[row] = count;
        if (rowSpecial) rowSpecial[row] = special;
    }
}

struct RectCopyArgs {
    float* field;      // [nz][ny][nx], first slice of the group
    float* box;        // [count][boxH][boxW]
    size_t total;      // nx * ny
    uint32_t nx, w, h, xa, ya;
    int back;
    uint32_t boxW, boxH, ox, oy;  // the rectangle sits at (ox, oy) of its box (fill2d pads rectangles to one size)
};
__global__ void __launch_bounds__(kBlock) rect_copy_kernel(RectCopyArgs a)
{
    const uint32_t y = blockIdx.x % a.h, s = blockIdx.x / a.h;
    float* src = a.field + (size_t)s * a.total + (size_t)(a.ya + y) * a.nx + a.xa;
    float* box = a.box + ((size_t)s * a.boxH + a.oy + y) * a.boxW + a.ox;
    for (uint32_t x = threadIdx.x; x < a.w; x += kBlock) {
        if (a.back) src[x] = box[x];
        else box[x] = src[x];
    }
}
// boxes [count][cells] filled with one value per box
__global__ void __launch_bounds__(kBlock) box_fill_kernel(float* __restrict__ box, size_t cells, const double* __restrict__ values)
{
    const float v = (float)values[blockIdx.y];
    float* b = box + (size_t)blockIdx.y * cells;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < cells; i += (size_t)gridDim.x * kBlock) b[i] = v;
}

// ---- what both drivers do first: bitmap, is it worth cutting, the rectangles per slice, the whole slices' statistics.
// fill2d: fields with defined cells that hold -0.0 or an infinity are not cut, and the boxes the rectangles are padded to must be
// worth it.  `fs` says which statistics (field, stats and total are filled in here).  false: take the whole slices (withHoles tells
// whether there was anything to cut at all); nothing has been written then.
struct RectCut {
    std::vector<std::vector<Rect>> rects;  // per slice
    std::vector<SliceStats> stats;         // of the whole slices: first guess, criterion, sweep bound, *nChanged
    std::vector<unsigned char> skip;       // SliceStats::skip: nothing defined or nothing undefined (:1266-1269, :1384-1386)
    size_t withHoles = 0;
};

bool cut_into_rects(size_t nx, size_t ny, size_t nz, const float* d_field, bool fill2d, FillStatsArgs fs, hipStream_t stream, RectCut& cut)
{
    const size_t total = nx * ny;
    const uint32_t words = (uint32_t)(ceil_div(nx, (size_t)64) * 2);
    DeviceArray<uint32_t> d_bits(nz * ny * words), d_rowCount((fill2d ? 2 : 1) * nz * ny);
    nan_bitmap_kernel<<<dim3((uint32_t)ceil_div(nz * ny, (size_t)(kBlock / kWave))), kBlock, 0, stream>>>(d_field, (uint32_t)nx, nz * ny, words, d_bits.get(), d_rowCount.get(),
                                                                                                     fill2d ? d_rowCount.get() + nz * ny : nullptr);
    FA_HIP(hipGetLastError());
    // first the rows' counts (a few KB): holes scattered over (nearly) all rows of a slice leave nothing to cut -- the usual case pays a pass
    // over the data on the device and this copy, not the bitmap's
    std::vector<uint32_t> rowCount(d_rowCount.size());
    FA_HIP(hipMemcpyAsync(rowCount.data(), d_rowCount.get(), rowCount.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    bool all = true;
    std::vector<unsigned char> consider(nz, 0);  // slices with undefined AND defined cells (the others are left alone)
    for (size_t z = 0; z < nz && all; ++z) {
        const int c = creep_rects::slice_candidate(rowCount.data() + z * ny, fill2d ? rowCount.data() + (nz + z) * ny : nullptr, ny, total);
        if (c == 0) continue;
        consider[z] = 1;
        cut.withHoles++;
        all = c > 0;
    }
    cut.rects.assign(nz, {});
    if (all && cut.withHoles != 0) {
        std::vector<uint32_t> bits(nz * ny * words);
        FA_HIP(hipMemcpyAsync(bits.data(), d_bits.get(), bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        for (size_t z = 0; z < nz && all; ++z) {
            if (!consider[z]) continue;
            all = slice_rects(bits.data() + z * ny * words, (uint32_t)nx, (uint32_t)ny, words, cut.rects[z]);
            if (all && fill2d) all = creep_rects::padded_boxes_worth_it(cut.rects[z], total);
        }
    }
    if (!all || cut.withHoles == 0) return false;
    DeviceArray<SliceStats> stats(nz);
    FA_HIP(hipMemsetAsync(stats.get(), 0, nz * sizeof(SliceStats), stream));
    fs.field = d_field;
    fs.stats = stats.get();
    fs.total = total;
    launch_fill_stats(fs, nz, stream);
    cut.stats.resize(nz);
    FA_HIP(hipMemcpyAsync(cut.stats.data(), stats.get(), nz * sizeof(SliceStats), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    cut.skip.resize(nz);
    for (size_t z = 0; z < nz; ++z) cut.skip[z] = cut.stats[z].skip != 0;
    return true;
}

// rectangle k of `rects` in slices z0 .. z0 + count - 1 of the field -> boxes [k][count][boxH][boxW], or back
void copy_rects(const char* what, float* d_field, size_t nx, size_t ny, size_t z0, size_t count, const std::vector<Rect>& rects, float* d_box,
                size_t boxW, size_t boxH, bool back, bool print, hipStream_t stream)
{
    for (size_t k = 0; k < rects.size(); ++k) {
        const Rect& q = rects[k];
        const size_t w = q.xb - q.xa + 1, h = q.yb - q.ya + 1;
        const std::pair<uint32_t, uint32_t> o = creep_rects::box_offset(q, nx, ny, boxW, boxH);
        if (kTuningBuild && !back && print)
            fprintf(stderr, "%s: slices %zu..%zu rectangle x %u..%u y %u..%u in boxes of %zu x %zu\n", what, z0, z0 + count - 1, q.xa, q.xb, q.ya, q.yb, boxW, boxH);
        RectCopyArgs c{d_field + z0 * nx * ny, d_box + k * count * boxW * boxH, nx * ny, (uint32_t)nx, (uint32_t)w, (uint32_t)h, q.xa, q.ya, back ? 1 : 0,
                       (uint32_t)boxW, (uint32_t)boxH, o.first, o.second};
        rect_copy_kernel<<<dim3((uint32_t)(count * h)), kBlock, 0, stream>>>(c);
        FA_HIP(hipGetLastError());
    }
}

// host values, one per slice of the run, repeated for each of `nr` rectangles -> device [nr][count]
template <typename T, typename F>
DeviceArray<T> per_box(size_t nr, size_t count, F value, hipStream_t stream, std::vector<T>& host)
{
    host.resize(nr * count);
    for (size_t k = 0; k < nr; ++k)
        for (size_t c = 0; c < count; ++c) host[k * count + c] = value(c);
    DeviceArray<T> d(nr * count);
    FA_HIP(hipMemcpyAsync(d.get(), host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return d;
}

}  // namespace

// Creep fill: rectangles of one size go through the sweeps together, as further slices of one run, and are copied back group by
// group (a rectangle's result does not depend on the others').
void run_creepfill(size_t nx, size_t ny, size_t nz, float* d_field, bool useDefault, float defaultVal,
                   unsigned short repeat, char setWeight, size_t* h_nChanged, hipStream_t stream)
{
    if (nx * ny == 0 || nz == 0) return;  // :1380
    auto whole = [&]() { run_creepfill_whole(nx, ny, nz, d_field, useDefault, defaultVal, repeat, setWeight, h_nChanged, stream, nullptr); };
    // worth looking for rectangles: large slices (the decomposition costs a pass over the data and a host round trip)
    const int mode = tuning("CREEP_RECTS", 1);  // 2 (tests): fail instead of falling back, 3 (tuning build): print the rectangles
    if (mode == 0 || nx < 64 || ny < 64 || nx > 0x7FFFFFFFu || ny > 0x7FFFFFFFu || nx * ny * nz > ((size_t)1 << 33)) {
        whole();
        return;
    }
    // the whole slices' statistics: the first guess (mean of the defined cells in scan order, :1502-1516) and *nChanged
    FillStatsArgs fs{};
    fs.useDefault = useDefault ? 1 : 0;
    fs.defaultVal = defaultVal;
    fs.sumAlgo = std::min(tuning("SUM_ALGO", 1), 1);
    RectCut cut;
    if (!cut_into_rects(nx, ny, nz, d_field, false, fs, stream, cut)) {
        FA_REQUIRE(mode != 2 || cut.withHoles == 0, "creepfill: CREEP_RECTS=2 (tests) asks for a field that can be cut into rectangles");
        whole();
        return;
    }
    for (size_t z = 0; z < nz; ++z)
        if (h_nChanged) h_nChanged[z] = (size_t)cut.stats[z].nUndef;
    for (size_t z0 = 0; z0 < nz;) {
        const size_t z1 = creep_rects::same_rects_run(cut.rects, cut.skip, z0, nz), count = z1 - z0;
        if (!cut.skip[z0]) {
            for (const std::vector<Rect>& same : creep_rects::rects_by_size(cut.rects[z0])) {
                const size_t w = same[0].xb - same[0].xa + 1, h = same[0].yb - same[0].ya + 1, boxes = same.size() * count;
                FA_REQUIRE(boxes * h <= 0x7FFFFFFFull, "creepfill: too many rows for one copy");
                DeviceArray<float> box(boxes * w * h);
                std::vector<double> hd;
                std::vector<unsigned long long> hb;  // the loop of a rectangle ends where the whole slice's would (:1430)
                const DeviceArray<double> d_def = per_box<double>(same.size(), count, [&](size_t c) { return cut.stats[z0 + c].average; }, stream, hd);
                const DeviceArray<unsigned long long> d_bnd =
                    per_box<unsigned long long>(same.size(), count, [&](size_t c) { return cut.stats[z0 + c].sweepBound; }, stream, hb);
                copy_rects("creepfill", d_field, nx, ny, z0, count, same, box.get(), w, h, false, mode == 3, stream);
                run_creepfill_whole(w, h, boxes, box.get(), true, 0.f, repeat, setWeight, nullptr, stream, d_def.get(), d_bnd.get());  // synchronises
                copy_rects("creepfill", d_field, nx, ny, z0, count, same, box.get(), w, h, true, false, stream);
                FA_HIP(hipStreamSynchronize(stream));  // box, hd, hb are released at the end of the iteration
            }
        }
        z0 = z1;
    }
    FA_HIP(hipStreamSynchronize(stream));
}

// fill2d by rectangles.  The same cut as for the creep fills (rows and columns that are defined throughout never change: w = 0,
// src/interpolation.c:1288-1315), with two differences.  The sweeps of the reference end by a criterion over the WHOLE field
// (:1338-1359), so the rectangles of a slice sweep in lock-step: they are padded to one size with defined cells (which change
// nothing), run as slices of ONE launch and end together by the criterion over all of them (Fill2dV2Args::couple).  And the
// reference's sweep adds e * 0 to every defined cell (:1327): that turns a -0.0 into +0.0 and, next to an infinity, a value into
// NaN -- fields with such defined cells are not cut.
void run_fill2d(size_t nx, size_t ny, size_t nz, float* d_field, float relaxCrit, float corrEff, size_t maxLoop,
                size_t* h_nChanged, hipStream_t stream)
{
    if (nx * ny == 0 || nz == 0) return;  // :1248
    auto whole = [&]() { (void)run_fill2d_whole(nx, ny, nz, d_field, relaxCrit, corrEff, maxLoop, h_nChanged, stream, nullptr, nullptr, 0); };
    const int mode = tuning("FILL_RECTS", 1);  // 2 (tests): fail instead of falling back, 3 (tuning build): print the rectangles
    if (mode == 0 || nx < 64 || ny < 64 || nx > 0x7FFFFFFFu || ny > 0x7FFFFFFFu || nx * ny * nz > ((size_t)1 << 33) || maxLoop == 0) {
        whole();
        return;
    }
    // the whole slices' statistics: first guess and criterion (:1281-1305), *nChanged
    FillStatsArgs fs{};
    fs.wantDeviation = 1;
    fs.relaxCrit = relaxCrit;
    fs.sumAlgo = 1;
    RectCut cut;
    if (!cut_into_rects(nx, ny, nz, d_field, true, fs, stream, cut)) {
        FA_REQUIRE(mode != 2 || cut.withHoles == 0, "fill2d: FILL_RECTS=2 (tests) asks for a field that can be cut into rectangles");
        whole();
        return;
    }
    // the boxes are filled before anything of the field is written: where a group cannot be launched, the whole call takes the other path
    struct Group { size_t z0, z1, mw, mh; DeviceArray<float> box; };
    std::vector<Group> groups;
    bool ok = true;
    const size_t cus = (size_t)device_cus();
    for (size_t z0 = 0; z0 < nz && ok;) {
        const std::vector<Rect>& rects = cut.rects[z0];
        // (the coupled boxes of a launch wait for each other: one workgroup per box at least, a CU each -- long batches go in several launches)
        const size_t z1 = creep_rects::same_rects_run(cut.rects, cut.skip, z0, std::max<size_t>(1, cus / std::max<size_t>(1, rects.size())));
        if (!cut.skip[z0] && !rects.empty()) {
            Group gr{z0, z1, 0, 0, {}};
            creep_rects::box_size(rects, gr.mw, gr.mh);
            const size_t count = z1 - z0, boxes = rects.size() * count, cells = gr.mw * gr.mh;
            ok = boxes * gr.mh <= 0x7FFFFFFFull && boxes <= 65535;
            if (!ok) break;
            gr.box.allocate(boxes * cells);
            std::vector<double> hd, hv;
            const DeviceArray<double> d_def = per_box<double>(rects.size(), count, [&](size_t c) { return cut.stats[z0 + c].average; }, stream, hd);
            const DeviceArray<double> d_dev = per_box<double>(rects.size(), count, [&](size_t c) { return cut.stats[z0 + c].meanAbsDev; }, stream, hv);
            box_fill_kernel<<<dim3((uint32_t)std::min<size_t>(ceil_div(cells, (size_t)kBlock), 1024), (uint32_t)boxes), kBlock, 0, stream>>>(gr.box.get(), cells, d_def.get());
            FA_HIP(hipGetLastError());
            copy_rects("fill2d", d_field, nx, ny, z0, count, rects, gr.box.get(), gr.mw, gr.mh, false, mode == 3, stream);
            ok = run_fill2d_whole(gr.mw, gr.mh, boxes, gr.box.get(), relaxCrit, corrEff, maxLoop, nullptr, stream, d_def.get(), d_dev.get(), (uint32_t)count);  // synchronises
            if (!ok) break;
            groups.push_back(std::move(gr));
        }
        z0 = z1;
    }
    if (!ok) {
        FA_REQUIRE(mode != 2, "fill2d: FILL_RECTS=2 (tests): a group of rectangles could not be launched");
        whole();
        return;
    }
    // copied back once every group has run: the field is untouched until then
    for (Group& gr : groups) copy_rects("fill2d", d_field, nx, ny, gr.z0, gr.z1 - gr.z0, cut.rects[gr.z0], gr.box.get(), gr.mw, gr.mh, true, false, stream);
    FA_HIP(hipStreamSynchronize(stream));
    for (size_t z = 0; z < nz; ++z)
        if (h_nChanged) h_nChanged[z] = (size_t)cut.stats[z].nUndef;
}

}  // namespace fimex_amd
