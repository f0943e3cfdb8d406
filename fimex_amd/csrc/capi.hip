// extern "C" boundary of libfimex_amd.so (include/fimex_amd.h), core: error channel, experiment switches, device selection, ABI
// version, caches.  The entry points live in capi_regrid.hip, capi_vector.hip, capi_fill.hip, capi_vertical.hip and
// capi_merge.hip; host_call.hpp carries one *_host call, capi_checks.hpp the shared argument checks.
#include "plan.hpp"

#include <cstdlib>
#include <cstring>
#include <string>

namespace fimex_amd {

namespace {
thread_local std::string g_lastError;
}

void set_last_error(const std::string& msg) { g_lastError = msg; }

// Experiment switches.  The product library does not read the environment: every switch has its
// measured default compiled in.  Only the tuning build (-DFIMEX_AMD_TUNING -> libfimex_amd_tuning.so, loaded by scripts/ and by
// the parity tests that force a fallback kernel) reads FIMEX_AMD_<NAME>, at every call so that one process can sweep settings.
int tuning(const char* name, int fallback)
{
#ifdef FIMEX_AMD_TUNING
    const std::string key = std::string("FIMEX_AMD_") + name;
    const char* v = std::getenv(key.c_str());
    if (!v || !*v) return fallback;
    const int parsed = std::atoi(v);
    return parsed < 0 ? fallback : parsed;
#else
    (void)name;
    return fallback;
#endif
}

namespace {

int usable_device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int usable = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) usable++;
    }
    return usable;
}

}  // namespace

int current_device_checked()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        throw Error("no HIP device: fimex_amd has no CPU fallback, an MI355X (gfx950) is required");
    }
    int dev = 0;
    FA_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    FA_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw Error(std::string("device is ") + prop.gcnArchName + ", the kernels are built for gfx950 only");
    return dev;
}

void require_current_device(int planDevice)
{
    int dev = 0;
    FA_HIP(hipGetDevice(&dev));
    FA_REQUIRE(dev == planDevice, "plan lives on device " + std::to_string(planDevice) +
                                      " but the calling thread's current device is " + std::to_string(dev));
}

}  // namespace fimex_amd

using namespace fimex_amd;

extern "C" {

const char* fimex_amd_last_error(void) { return g_lastError.c_str(); }

int fimex_amd_release_caches(void)
{
    return c_guard([&] { release_host_pipes(); });
}

int fimex_amd_abi_version(void) { return 131; }  // 1.31: source and output batches placed by the library, the gather cross-check

int fimex_amd_device_count(void) { return usable_device_count(); }

int fimex_amd_set_device(int ordinal)
{
    return c_guard([&] {
        FA_HIP(hipSetDevice(ordinal));
        (void)current_device_checked();
    });
}

}  // extern "C"
