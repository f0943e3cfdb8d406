// extern "C" boundary, regridding: plans, apply and gather, tuning, batches, the typed apply, regrid_slice and the conversions
// between stored types and the float form the kernels interpolate.
#include "host_call.hpp"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

namespace fimex_amd {

void apply_plan_device(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream)
{
    if (plan.kind == PlanKind::Forward) launch_forward_apply(plan, d_in, nz, d_out, stream);
    else launch_backward_apply(plan, d_in, nz, d_out, stream);
}

// on the stored type: one kernel where launch_typed_apply has one, the three passes on temporaries otherwise
void apply_plan_typed_device(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                             hipStream_t st)
{
    if (launch_typed_apply(plan, d_in, cdmType, nz, badValue, d_out, st)) return;
    const size_t inLayer = plan.inX * plan.inY, outLayer = plan.outX * plan.outY;
    DeviceArray<float> fIn(nz * inLayer), fOut(nz * outLayer);
    launch_data2interpolation(d_in, cdmType, nz * inLayer, badValue, fIn.get(), st);
    apply_plan_device(plan, fIn.get(), nz, fOut.get(), st);
    launch_interpolation2data(fOut.get(), nz * outLayer, cdmType, badValue, d_out, st);
    FA_HIP(hipStreamSynchronize(st));  // the temporaries are released on return
}

namespace {

bool is_backward(int funcType)
{
    return funcType == FIMEX_AMD_INTERPOL_NEAREST_NEIGHBOR || funcType == FIMEX_AMD_INTERPOL_BILINEAR ||
           funcType == FIMEX_AMD_INTERPOL_BICUBIC || funcType == FIMEX_AMD_INTERPOL_COORD_NN ||
           funcType == FIMEX_AMD_INTERPOL_COORD_NN_KD;
}

bool is_forward(int funcType)
{
    return funcType >= FIMEX_AMD_INTERPOL_FORWARD_SUM && funcType <= FIMEX_AMD_INTERPOL_FORWARD_UNDEF_MIN;
}

std::unique_ptr<fimex_amd_regrid_plan> new_plan(int funcType, size_t nPoints, size_t inX, size_t inY, size_t outX, size_t outY)
{
    // same failure as CachedInterpolation.cc:114 / CachedForwardInterpolation.cc:88
    FA_REQUIRE(is_backward(funcType) || is_forward(funcType), "unknown interpolation function: " + std::to_string(funcType));
    auto plan = std::make_unique<fimex_amd_regrid_plan>();
    plan->funcType = funcType;
    plan->inX = inX;
    plan->inY = inY;
    plan->outX = outX;
    plan->outY = outY;
    if (is_backward(funcType)) {
        plan->kind = funcType == FIMEX_AMD_INTERPOL_BILINEAR ? PlanKind::Bilinear
                   : funcType == FIMEX_AMD_INTERPOL_BICUBIC  ? PlanKind::Bicubic
                                                             : PlanKind::Nearest;
        FA_REQUIRE(nPoints == outX * outY, "backward plans need one position per output cell (outX*outY)");
    } else {
        plan->kind = PlanKind::Forward;
        const int k = (funcType - FIMEX_AMD_INTERPOL_FORWARD_SUM) % 5;
        plan->aggregate = static_cast<Aggregate>(k);  // sum, mean, median, max, min
        plan->undefAggr = funcType >= FIMEX_AMD_INTERPOL_FORWARD_UNDEF_SUM;
        FA_REQUIRE(nPoints == inX * inY, "forward plans need one position per input cell (inX*inY)");
    }
    plan->device = current_device_checked();
    plan->info.funcType = funcType;
    plan->info.device = plan->device;
    plan->info.inX = inX;
    plan->info.inY = inY;
    plan->info.outX = outX;
    plan->info.outY = outY;
    return plan;
}

void build_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream)
{
    if (plan.kind == PlanKind::Forward) build_forward_plan(plan, d_px, d_py, stream);
    else build_backward_plan(plan, d_px, d_py, stream);
}

// data2interpolation / interpolation2data, on the caller's device buffers or on copies of the caller's host arrays
template <class Call>
void data2interpolation(Call&& c, const void* in, int cdmType, size_t n, double badValue, float* out, const char* nullArray)
{
    const size_t elem = cdm_type_size(cdmType);
    if (n == 0) return;
    FA_REQUIRE(in != nullptr && out != nullptr, nullArray);
    (void)current_device_checked();
    launch_data2interpolation(c.in_bytes(in, n * elem), cdmType, n, badValue, c.out(out, n), c.stream());
    c.finish();
}

template <class Call>
void interpolation2data(Call&& c, const float* in, size_t n, int cdmType, double badValue, void* out, const char* nullArray)
{
    const size_t elem = cdm_type_size(cdmType);
    if (n == 0) return;
    FA_REQUIRE(in != nullptr && out != nullptr, nullArray);
    (void)current_device_checked();
    launch_interpolation2data(c.in(in, n), n, cdmType, badValue, c.out_bytes(out, n * elem), c.stream());
    c.finish();
}

}  // namespace
}  // namespace fimex_amd

using namespace fimex_amd;

extern "C" {

int fimex_amd_regrid_plan_create(int funcType, const double* px, const double* py, size_t nPoints, size_t inX, size_t inY,
                                 size_t outX, size_t outY, fimex_amd_regrid_plan** out)
{
    return fimex_amd_regrid_plan_create_opt(funcType, px, py, nPoints, inX, inY, outX, outY, FIMEX_AMD_BICUBIC_REFERENCE, out);
}

int fimex_amd_regrid_plan_create_device(int funcType, const double* d_px, const double* d_py, size_t nPoints, size_t inX,
                                        size_t inY, size_t outX, size_t outY, void* stream, fimex_amd_regrid_plan** out)
{
    return fimex_amd_regrid_plan_create_device_opt(funcType, d_px, d_py, nPoints, inX, inY, outX, outY, FIMEX_AMD_BICUBIC_REFERENCE, stream, out);
}

static void set_arithmetic(fimex_amd_regrid_plan& plan, int bicubicArithmetic)
{
    FA_REQUIRE(bicubicArithmetic == FIMEX_AMD_BICUBIC_REFERENCE || bicubicArithmetic == FIMEX_AMD_BICUBIC_FAST,
               "unknown bicubic arithmetic: " + std::to_string(bicubicArithmetic));
    plan.bicubicFast = plan.kind == PlanKind::Bicubic && bicubicArithmetic == FIMEX_AMD_BICUBIC_FAST;
}

int fimex_amd_regrid_plan_create_opt(int funcType, const double* px, const double* py, size_t nPoints, size_t inX, size_t inY,
                                     size_t outX, size_t outY, int bicubicArithmetic, fimex_amd_regrid_plan** out)
{
    return c_guard([&] {
        FA_REQUIRE(out != nullptr, "plan output pointer is NULL");
        *out = nullptr;
        FA_REQUIRE(px != nullptr && py != nullptr, "position arrays are NULL");
        auto plan = new_plan(funcType, nPoints, inX, inY, outX, outY);
        set_arithmetic(*plan, bicubicArithmetic);
        HostCall hc;
        build_plan(*plan, hc.in(px, nPoints), hc.in(py, nPoints), hc.stream());
        hc.finish();
        *out = plan.release();
    });
}

int fimex_amd_regrid_plan_create_device_opt(int funcType, const double* d_px, const double* d_py, size_t nPoints, size_t inX,
                                            size_t inY, size_t outX, size_t outY, int bicubicArithmetic, void* stream,
                                            fimex_amd_regrid_plan** out)
{
    return c_guard([&] {
        FA_REQUIRE(out != nullptr, "plan output pointer is NULL");
        *out = nullptr;
        FA_REQUIRE(d_px != nullptr && d_py != nullptr, "position arrays are NULL");
        auto plan = new_plan(funcType, nPoints, inX, inY, outX, outY);
        set_arithmetic(*plan, bicubicArithmetic);
        build_plan(*plan, d_px, d_py, as_stream(stream));
        *out = plan.release();
    });
}

int fimex_amd_regrid_plan_destroy(fimex_amd_regrid_plan* plan)
{
    return c_guard([&] {
        if (!plan) return;
        ScopedDevice dev(plan->device);
        delete plan;
    });
}

int fimex_amd_regrid_plan_info(const fimex_amd_regrid_plan* plan, fimex_amd_plan_info* info)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && info != nullptr, "NULL argument");
        *info = plan->info;
    });
}

// not a plain round trip: the size query, and slices streamed through pinned staging where that pays
int fimex_amd_regrid_apply_host(const fimex_amd_regrid_plan* plan, const float* inData, size_t size, float* outData,
                                size_t outCapacity, size_t* newSize)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && newSize != nullptr, "NULL argument");
        const size_t inLayer = plan->inX * plan->inY, outLayer = plan->outX * plan->outY;
        const size_t nz = size / inLayer;  // CachedInterpolation.cc:121
        *newSize = outLayer * nz;          // :122
        if (outData == nullptr) return;    // size query
        FA_REQUIRE(inData != nullptr || nz == 0, "inData is NULL");
        FA_REQUIRE(outCapacity >= *newSize, "output buffer too small");
        if (nz == 0) return;
        ScopedDevice dev(plan->device);
        // slices are independent: stream them through pinned staging, transfers overlapping the kernels
        if (pipelined_slices(plan->device, inData, inLayer * sizeof(float), outData, outLayer * sizeof(float), 0, 0, nz,
                             [&](const void* dIn, void* dOut, float*, float*, size_t nzc, hipStream_t st) {
                                 apply_plan_device(*plan, static_cast<const float*>(dIn), nzc, static_cast<float*>(dOut), st);
                             }))
            return;
        HostCall hc;
        apply_plan_device(*plan, hc.in(inData, nz * inLayer), nz, hc.out(outData, nz * outLayer), hc.stream());
        hc.finish();
    });
}

int fimex_amd_regrid_apply_device(const fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, float* d_out, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        if (nz == 0) return;
        FA_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL device buffer");
        require_current_device(plan->device);
        apply_plan_device(*plan, d_in, nz, d_out, as_stream(stream));
    });
}

int fimex_amd_regrid_plan_tune_device(fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, float* d_out, void* stream, int* chosenShape)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        if (chosenShape) *chosenShape = plan->useAlt;
        // nothing to choose between: a batch that takes the gather kernels anyway, or neither a second shape nor a batch long enough
        // for the second launch order (the choices made on a longer batch stay as they are).  A batch that has two shapes but is too
        // short for the second order chooses the shape again and leaves the order alone: its own launches do not read it.
        const bool shapes = plan->staged2Alt.valid;
        const dispatch::Switches sw = dispatch_switches();
        const bool orders = dispatch::float_apply(sw, plan_facts(*plan), nz) == dispatch::FloatApply::Second &&
                            chunk_xcd_chunk_count(nz, staged2_zpb()) != 0;
        if (!dispatch::tune_has_choice(sw, plan_facts(*plan), nz, shapes, orders)) return;
        FA_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL device buffer");
        require_current_device(plan->device);
        hipStream_t st = as_stream(stream);
        ScopedEvent e0, e1;
        struct DefaultShapeOnError {  // a failed timing leaves the default shape and order selected
            fimex_amd_regrid_plan* plan;
            ~DefaultShapeOnError() { if (plan) plan->useAlt = plan->chunkXcd = 0; }
        } onError{plan};
        if (orders) plan->chunkXcd = 0;  // the shapes are timed in the default order
        auto median_ms = [&] {
            std::vector<float> ms;
            for (int rep = 0; rep < 7; ++rep) {  // two launches to settle, five timed: the median counts
                FA_HIP(hipEventRecord(e0.e, st));
                apply_plan_device(*plan, d_in, nz, d_out, st);
                FA_HIP(hipEventRecord(e1.e, st));
                FA_HIP(hipEventSynchronize(e1.e));
                float t = 0.f;
                FA_HIP(hipEventElapsedTime(&t, e0.e, e1.e));
                if (rep >= 2) ms.push_back(t);
            }
            std::sort(ms.begin(), ms.end());
            return ms[ms.size() / 2];
        };
        float best[2] = {0.f, 0.f};
        for (int shape = 0; shape < (shapes ? 2 : 1); ++shape) {
            plan->useAlt = shape;
            best[shape] = median_ms();
        }
        plan->useAlt = shapes && best[1] < 0.99f * best[0] ? 1 : 0;  // the default shape unless the other one is clearly faster
        if (orders) {  // then the chunk-per-XCD order on the winning shape, by the same rule
            plan->chunkXcd = 1;
            plan->chunkXcd = median_ms() < 0.99f * best[plan->useAlt] ? 1 : 0;
        }
        onError.plan = nullptr;
        plan->info.launchOrder = (size_t)plan->chunkXcd;
        const auto& s = plan->useAlt ? plan->staged2Alt : plan->staged2;
        plan->info.planBytes = plan->planBytesShape[plan->useAlt];
        plan->info.stagedCells = s.stagedCells;
        plan->info.tileW = s.tileWMax;
        plan->info.tileH = s.tileH;
        if (chosenShape) *chosenShape = plan->useAlt;
    });
}

int fimex_amd_regrid_plan_launch_order(const fimex_amd_regrid_plan* plan, size_t nz, int* order)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && order != nullptr, "NULL argument");
        *order = plan->kind == PlanKind::Forward ? -1 : backward_launch_order(*plan, nz);
    });
}

int fimex_amd_regrid_apply_gather_device(const fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, float* d_out, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        FA_REQUIRE(plan->kind != PlanKind::Forward, "the gather kernels serve backward plans");
        if (nz == 0) return;
        FA_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL device buffer");
        require_current_device(plan->device);
        launch_backward_gather(*plan, d_in, nz, d_out, as_stream(stream));
    });
}

int fimex_amd_regrid_batch_alloc_device(const fimex_amd_regrid_plan* plan, const float* d_in, size_t nz, int positions, void* stream,
                                        fimex_amd_batch** batch)
{
    return c_guard([&] {
        FA_REQUIRE(batch != nullptr, "batch output pointer is NULL");
        *batch = nullptr;
        FA_REQUIRE(plan != nullptr, "NULL plan");
        require_current_device(plan->device);
        *batch = batch_alloc(*plan, d_in, nz, positions, as_stream(stream));
    });
}

int fimex_amd_regrid_source_batch_alloc_device(const fimex_amd_regrid_plan* plan, size_t nz, int candidates, void* stream, fimex_amd_batch** batch)
{
    return c_guard([&] {
        FA_REQUIRE(batch != nullptr, "batch output pointer is NULL");
        *batch = nullptr;
        FA_REQUIRE(plan != nullptr, "NULL plan");
        require_current_device(plan->device);
        *batch = batch_alloc_source(*plan, nz, candidates, as_stream(stream));
    });
}

int fimex_amd_batch_get_info(const fimex_amd_batch* batch, fimex_amd_batch_info* info)
{
    return c_guard([&] {
        FA_REQUIRE(batch != nullptr && info != nullptr, "NULL argument");
        *info = batch_info(*batch);
    });
}

int fimex_amd_batch_free(fimex_amd_batch* batch)
{
    return c_guard([&] { batch_free(batch); });
}

int fimex_amd_bad2nan_device(float* d_data, size_t n, float badVal, void* stream)
{
    return c_guard([&] {
        if (n == 0) return;
        FA_REQUIRE(d_data != nullptr, "NULL device buffer");
        (void)current_device_checked();
        launch_bad2nan(d_data, n, badVal, as_stream(stream));
    });
}

int fimex_amd_nan2bad_device(float* d_data, size_t n, float badVal, void* stream)
{
    return c_guard([&] {
        if (n == 0) return;
        FA_REQUIRE(d_data != nullptr, "NULL device buffer");
        (void)current_device_checked();
        launch_nan2bad(d_data, n, badVal, as_stream(stream));
    });
}

namespace {

// CDMInterpolator::getDataSlice, src/CDMInterpolator.cc:251-285, on one step of one variable; typed == false is the
// float-in / float-out form (conversions reduced to mifi_bad2nanf / mifi_nanf2bad with a float fill value)
void regrid_slice(const fimex_amd_regrid_plan* plan, bool typed, const void* inData, int dataType, size_t size, double badValue,
                  const fimex_amd_process2d* pre, size_t nPre, const void* counterpart, int counterpartType,
                  double badValueCounterpart, const fimex_amd_vector_plan* vec, int isXComponent,
                  const fimex_amd_process2d* post, size_t nPost, void* outData, size_t outCapacity, size_t* newSize)
{
    FA_REQUIRE(plan != nullptr && newSize != nullptr, "NULL argument");
    FA_REQUIRE((nPre == 0 || pre != nullptr) && (nPost == 0 || post != nullptr), "NULL process list");
    const size_t inLayer = plan->inX * plan->inY, outLayer = plan->outX * plan->outY;
    const size_t nz = size / inLayer;
    *newSize = outLayer * nz;
    if (outData == nullptr) return;
    FA_REQUIRE(outCapacity >= *newSize, "output buffer too small");
    const size_t elem = typed ? cdm_type_size(dataType) : sizeof(float);
    if (nz == 0) return;
    FA_REQUIRE(inData != nullptr, "inData is NULL");
    const bool vector = counterpart != nullptr && vec != nullptr;
    if (vector) FA_REQUIRE(vec->device == plan->device && vec->ox == plan->outX && vec->oy == plan->outY,
                           "vector reprojection does not match the regrid plan");
    const size_t elemOther = (vector && typed) ? cdm_type_size(counterpartType) : sizeof(float);
    ScopedDevice dev(plan->device);
    if (!vector && nPre == 0 && nPost == 0) {
        // conversion, regrid, conversion per chunk of slices, transfers streamed
        const bool convert = typed && dataType != FIMEX_AMD_CDM_FLOAT;
        if (pipelined_slices(plan->device, inData, inLayer * elem, outData, outLayer * elem, convert ? inLayer : 0, typed ? outLayer : 0, nz,
                             [&](const void* dIn, void* dOut, float* fIn, float* fOut, size_t nzc, hipStream_t st) {
                                 if (typed && launch_typed_apply(*plan, dIn, dataType, nzc, badValue, dOut, st)) return;
                                 const float* src = static_cast<const float*>(dIn);
                                 if (convert) {
                                     launch_data2interpolation(dIn, dataType, nzc * inLayer, badValue, fIn, st);
                                     src = fIn;
                                 } else {
                                     launch_bad2nan(const_cast<float*>(src), nzc * inLayer, (float)badValue, st);  // staging copy, not the caller's
                                 }
                                 if (typed) {
                                     apply_plan_device(*plan, src, nzc, fOut, st);
                                     launch_interpolation2data(fOut, nzc * outLayer, dataType, badValue, dOut, st);
                                 } else {
                                     apply_plan_device(*plan, src, nzc, static_cast<float*>(dOut), st);
                                     launch_nan2bad(static_cast<float*>(dOut), nzc * outLayer, (float)badValue, st);
                                 }
                             }))
            return;
    }
    // not a round trip: a component's upload buffers are released before the next one is regridded, so the stream is waited for
    // in between
    ScopedStream stream;
    hipStream_t st = stream.get();
    auto run = [&](const fimex_amd_process2d* list, size_t n, float* d, size_t nx, size_t ny) {
        for (size_t i = 0; i < n; ++i) {
            const fimex_amd_process2d& p = list[i];
            switch (p.kind) {
            case FIMEX_AMD_PROCESS_FILL2D: run_fill2d(nx, ny, nz, d, p.relaxCrit, p.corrEff, p.maxLoop, nullptr, st); break;
            case FIMEX_AMD_PROCESS_CREEPFILL2D: run_creepfill(nx, ny, nz, d, false, 0.f, p.repeat, p.setWeight, nullptr, st); break;
            case FIMEX_AMD_PROCESS_CREEPFILLVAL2D: run_creepfill(nx, ny, nz, d, true, p.defaultVal, p.repeat, p.setWeight, nullptr, st); break;
            default: throw Error("unknown 2-D process kind " + std::to_string(p.kind));
            }
        }
    };
    // one component: upload in its stored type, -> float with the fill value as NaN, pre-processes, regrid
    auto regrid = [&](const void* h_in, int type, size_t bytesPerElem, double bad, DeviceArray<float>& d_out) {
        DeviceArray<float> d_in(nz * inLayer);
        DeviceArray<unsigned char> d_raw;
        if (typed && type != FIMEX_AMD_CDM_FLOAT) {
            d_raw.allocate(nz * inLayer * bytesPerElem);
            host_to_device(d_raw.get(), h_in, d_raw.bytes(), st);
            launch_data2interpolation(d_raw.get(), type, d_in.size(), bad, d_in.get(), st);
        } else {
            host_to_device(d_in.get(), h_in, d_in.bytes(), st);
            launch_bad2nan(d_in.get(), d_in.size(), (float)bad, st);
        }
        run(pre, nPre, d_in.get(), plan->inX, plan->inY);
        d_out.allocate(nz * outLayer);
        apply_plan_device(*plan, d_in.get(), nz, d_out.get(), st);
        FA_HIP(hipStreamSynchronize(st));  // d_in / d_raw are released on return
    };
    DeviceArray<float> d_main, d_other;
    regrid(inData, dataType, elem, badValue, d_main);
    if (vector) {
        regrid(counterpart, counterpartType, elemOther, badValueCounterpart, d_other);
        if (isXComponent) launch_vector_values(*vec, d_main.get(), d_other.get(), nz, st);
        else launch_vector_values(*vec, d_other.get(), d_main.get(), nz, st);
    }
    run(post, nPost, d_main.get(), plan->outX, plan->outY);
    if (typed) {
        DeviceArray<unsigned char> d_typed(d_main.size() * elem);
        launch_interpolation2data(d_main.get(), d_main.size(), dataType, badValue, d_typed.get(), st);
        device_to_host(outData, d_typed.get(), d_typed.bytes(), st);
        stream.sync();
    } else {
        launch_nan2bad(d_main.get(), d_main.size(), (float)badValue, st);
        device_to_host(outData, d_main.get(), d_main.bytes(), st);
        stream.sync();
    }
}

}  // namespace

int fimex_amd_regrid_slice_host(const fimex_amd_regrid_plan* plan, const float* inData, size_t size, float badValue,
                                const fimex_amd_process2d* pre, size_t nPre, const float* counterpart,
                                float badValueCounterpart, const fimex_amd_vector_plan* vec, int isXComponent,
                                const fimex_amd_process2d* post, size_t nPost, float* outData, size_t outCapacity,
                                size_t* newSize)
{
    return c_guard([&] {
        regrid_slice(plan, false, inData, FIMEX_AMD_CDM_FLOAT, size, badValue, pre, nPre, counterpart, FIMEX_AMD_CDM_FLOAT,
                     badValueCounterpart, vec, isXComponent, post, nPost, outData, outCapacity, newSize);
    });
}

int fimex_amd_regrid_slice_typed_host(const fimex_amd_regrid_plan* plan, const void* inData, int dataType, size_t size, double badValue,
                                      const fimex_amd_process2d* pre, size_t nPre, const void* counterpart, int counterpartType,
                                      double badValueCounterpart, const fimex_amd_vector_plan* vec, int isXComponent,
                                      const fimex_amd_process2d* post, size_t nPost, void* outData, size_t outCapacity,
                                      size_t* newSize)
{
    return c_guard([&] {
        regrid_slice(plan, true, inData, dataType, size, badValue, pre, nPre, counterpart, counterpartType, badValueCounterpart,
                     vec, isXComponent, post, nPost, outData, outCapacity, newSize);
    });
}

int fimex_amd_data2interpolation_device(const void* d_in, int cdmType, size_t n, double badValue, float* d_out, void* stream)
{
    return c_guard([&] { data2interpolation(DeviceCall{as_stream(stream)}, d_in, cdmType, n, badValue, d_out, "NULL device buffer"); });
}

int fimex_amd_data2interpolation_host(const void* in, int cdmType, size_t n, double badValue, float* out)
{
    return c_guard([&] { data2interpolation(HostCall(), in, cdmType, n, badValue, out, "NULL argument"); });
}

int fimex_amd_interpolation2data_device(const float* d_in, size_t n, int cdmType, double badValue, void* d_out, void* stream)
{
    return c_guard([&] { interpolation2data(DeviceCall{as_stream(stream)}, d_in, n, cdmType, badValue, d_out, "NULL device buffer"); });
}

int fimex_amd_interpolation2data_host(const float* in, size_t n, int cdmType, double badValue, void* out)
{
    return c_guard([&] { interpolation2data(HostCall(), in, n, cdmType, badValue, out, "NULL argument"); });
}

int fimex_amd_regrid_apply_typed_device(const fimex_amd_regrid_plan* plan, const void* d_in, int cdmType, size_t nz, double badValue,
                                        void* d_out, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        (void)cdm_type_size(cdmType);
        if (nz == 0) return;
        FA_REQUIRE(d_in != nullptr && d_out != nullptr, "NULL device buffer");
        ScopedDevice dev(plan->device);
        apply_plan_typed_device(*plan, d_in, cdmType, nz, badValue, d_out, as_stream(stream));
    });
}

}  // extern "C"
