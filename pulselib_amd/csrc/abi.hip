// abi.hip -- error reporting, the launch helpers every unit shares, and version of libpulse_hip.so (include/pulse_env.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "pulse_internal.h"

namespace {
thread_local char g_err[512] = "";
}

namespace pulse {

int fail(int code, const char* msg) {
    std::snprintf(g_err, sizeof g_err, "%s", msg ? msg : "");
    return code;
}

int fail_hip(int hip_error, const char* what) {
    const hipError_t e = (hipError_t)hip_error;
    std::snprintf(g_err, sizeof g_err, "%s: HIP error %d (%s)", what ? what : "hip", hip_error, hipGetErrorString(e));
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNotInitialized) ? PULSE_ENODEVICE : PULSE_ELAUNCH;
}

LdsLaunch launch_lds(const void* fn, unsigned grid, unsigned block, void** params, size_t lds_bytes, ihipStream_t* stream, bool launch_if_refused) {
    hipError_t attr = hipSuccess;
    if (lds_bytes > 48 * 1024) {
        // Assumes what the three tables this one replaces assumed: one launching thread (no lock) and one device per process
        // (the limit is a property of the function on a device; the table is keyed by function alone).
        static struct { const void* fn; size_t bytes; } raised[64] = {};     // (the library has some thirty such kernel instances)
        int i = 0;
        while (i < 64 && raised[i].fn && raised[i].fn != fn) ++i;
        if (i == 64 || raised[i].bytes < lds_bytes) {
            attr = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (attr == hipSuccess && i < 64) { raised[i].fn = fn; raised[i].bytes = lds_bytes; }
        }
    }
    if (attr != hipSuccess && !launch_if_refused) return {(int)attr, (int)hipSuccess};
    if (attr != hipSuccess) (void)hipGetLastError();      // the launch below reports what is wrong, not the attribute call's sticky error
    return {(int)attr, (int)hipLaunchKernel(fn, dim3(grid), dim3(block), params, lds_bytes, stream)};
}

int resident_blocks_per_cu(const void* fn, int block, size_t lds_bytes) {
    // the assumptions of launch_lds's table, except that the device is part of the key (a partition holds fewer)
    static struct { const void* fn; size_t bytes; int dev, per_cu; } asked[64] = {};
    int dev = 0, per_cu = 0, i = 0;
    hipError_t e = hipGetDevice(&dev);
    while (i < 64 && asked[i].fn && !(asked[i].fn == fn && asked[i].bytes == lds_bytes && asked[i].dev == dev)) ++i;
    if (e == hipSuccess && i < 64 && asked[i].fn) return asked[i].per_cu;
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, lds_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail_hip((int)e, "occupancy query"); }
    if (per_cu < 0) per_cu = 0;
    if (i < 64) asked[i] = {fn, lds_bytes, dev, per_cu};
    return per_cu;
}

long long* CalledOffWord::get() {
    void* p = nullptr;
    if (!word && hipHostMalloc(&p, sizeof(long long), hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) (void)hipGetLastError();
    if (!word && p) { word = static_cast<long long*>(p); *word = 0; }
    return word;
}
long long CalledOffWord::count() const { return word ? __atomic_load_n(word, __ATOMIC_ACQUIRE) : 0; }
bool CalledOffWord::changed() { const long long was = seen; seen = count(); return seen != was; }

}  // namespace pulse

// ---- the tail of an entry point, one copy for every unit (pulse_internal.h)
int pulse::fail_named(const char* name, const char* msg) {
    char text[256];
    std::snprintf(text, sizeof text, "%s: %s", name, msg);
    return fail(PULSE_EINVAL, text);
}

int pulse::finish_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip((int)e, what);
    return 0;
}

int pulse::device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    if (cus[dev] == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus[dev] = prop.multiProcessorCount;
        else { (void)hipGetLastError(); cus[dev] = 256; }
    }
    return cus[dev];
}

extern "C" {

int pulse_version(void) { return PULSE_ABI_VERSION; }

const char* pulse_last_error(void) { return g_err; }

}  // extern "C"
