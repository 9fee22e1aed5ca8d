// What sx_launch.hpp declares: the sampled kernel timer (sx_profile_*), the launch check, the dynamic-LDS grant and the
// device's compute-unit count -- one copy of their state for every translation unit of libsxamd -- and sx_version.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/sx_amd.h"
#include "sx_launch.hpp"

namespace sx {

// ---------------------------------------------------------------------------------------------------------------
// Optional kernel timer (sx_profile_*): while enabled, every n-th launch of each of the path's kernel classes carries a
// pair of HIP events on the stream the kernel is launched on (sx_launch.hpp); sx_profile_collect adds the elapsed times up
// per kernel class.
// This is how bench.py measures `roofline.avg_launch_us` live, inside its timed region.
// ---------------------------------------------------------------------------------------------------------------
struct ProfEntry {
    int kind;
    hipEvent_t start, stop;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static size_t g_prof_cap = 0;
static int g_prof_stride[SX_PROF_KINDS] = {1, 1, 1, 1, 1, 1, 1};   // every n-th launch of a kernel class is timed
static long g_prof_seen[SX_PROF_KINDS] = {0};
static std::vector<ProfEntry> g_prof_entries;
static std::vector<hipEvent_t> g_prof_pool;

// Takes a (start, stop) event pair for one launch of kernel class `kind`, or returns false (timer off / cap reached).
bool prof_take(int kind, hipEvent_t* start, hipEvent_t* stop) {
    if (!g_prof_on) return false;   // (read without the lock: enabling mid-launch only loses that launch)
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (!g_prof_on || g_prof_entries.size() >= g_prof_cap) return false;
    if ((g_prof_seen[kind]++ % g_prof_stride[kind]) != 0) return false;
    auto take = [&]() {
        hipEvent_t e = nullptr;
        if (!g_prof_pool.empty()) {
            e = g_prof_pool.back();
            g_prof_pool.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    };
    hipEvent_t a = take(), b = take();
    if (!a || !b) return false;
    g_prof_entries.push_back(ProfEntry{kind, a, b});
    *start = a;
    *stop = b;
    return true;
}

// (launch<>() -- every kernel of the path is launched through it -- and allow_lds<>() live in sx_launch.hpp, which every
// translation unit with a launcher includes.)
int check_launch() {
    // SX_DEBUG_SYNC=1: wait for the launch and report an asynchronous failure at the call that caused it (diagnosis only)
    static const bool debug_sync = std::getenv("SX_DEBUG_SYNC") != nullptr;
    if (debug_sync) {
        const hipError_t serr = hipDeviceSynchronize();
        if (serr != hipSuccess) {
            std::fprintf(stderr, "libsxamd: kernel failed: %s\n", hipGetErrorString(serr));
            return SX_ERR_LAUNCH;
        }
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        std::fprintf(stderr, "libsxamd: HIP launch error: %s\n", hipGetErrorString(err));
        return SX_ERR_LAUNCH;
    }
    return SX_OK;
}


// Kernels that need more than 64 KB of dynamic LDS must be granted it once per (device, kernel); the grant is remembered,
// so the hot loop's launches make no runtime call besides the launch itself.
int allow_lds_ptr(const void* kernel, size_t bytes) {
    if (bytes > kMaxLdsBytes) return SX_ERR_UNSUPPORTED;
    if (bytes > 64 * 1024) {
        static std::mutex mu;
        static std::map<std::pair<int, const void*>, size_t> granted;
        int dev = 0;
        (void)hipGetDevice(&dev);
        const auto key = std::make_pair(dev, kernel);
        std::lock_guard<std::mutex> lock(mu);
        auto it = granted.find(key);
        if (it != granted.end() && it->second >= bytes) return SX_OK;
        if (hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            (void)hipGetLastError();
            return SX_ERR_UNSUPPORTED;
        }
        granted[key] = bytes;
    }
    return SX_OK;
}

// compute units of the current device (the persistent grids are sized by it)
int device_cus() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
    return n;
}

}  // namespace sx

extern "C" {

const char* sx_version(void) { return "sxamd 0.3 gfx950"; }

int sx_profile_enable(int max_launches) {
    if (max_launches <= 0) return SX_ERR_ARG;
    std::lock_guard<std::mutex> lock(sx::g_prof_mu);
    for (auto& e : sx::g_prof_entries) {
        sx::g_prof_pool.push_back(e.start);
        sx::g_prof_pool.push_back(e.stop);
    }
    sx::g_prof_entries.clear();
    sx::g_prof_cap = (size_t)max_launches;
    for (long& n : sx::g_prof_seen) n = 0;
    sx::g_prof_on = true;
    return SX_OK;
}

int sx_profile_stride(int every) {
    if (every <= 0) return SX_ERR_ARG;
    std::lock_guard<std::mutex> lock(sx::g_prof_mu);
    for (int& v : sx::g_prof_stride) v = every;
    return SX_OK;
}

int sx_profile_stride_kind(int kind, int every) {
    if (every <= 0 || kind < 0 || kind >= SX_PROF_KINDS) return SX_ERR_ARG;
    std::lock_guard<std::mutex> lock(sx::g_prof_mu);
    sx::g_prof_stride[kind] = every;
    return SX_OK;
}

int sx_profile_collect(int kind, double* total_ms, int64_t* launches) {
    if (kind < 0 || kind >= SX_PROF_KINDS || !total_ms || !launches) return SX_ERR_ARG;
    std::lock_guard<std::mutex> lock(sx::g_prof_mu);
    double tot = 0.0;
    int64_t n = 0;
    for (auto& e : sx::g_prof_entries) {
        if (e.kind != kind) continue;
        float ms = 0.f;
        if (hipEventSynchronize(e.stop) != hipSuccess || hipEventElapsedTime(&ms, e.start, e.stop) != hipSuccess) {
            (void)hipGetLastError();
            return SX_ERR_LAUNCH;
        }
        tot += ms;
        ++n;
    }
    *total_ms = tot;
    *launches = n;
    return SX_OK;
}

int sx_profile_disable(void) {
    std::lock_guard<std::mutex> lock(sx::g_prof_mu);
    sx::g_prof_on = false;
    for (auto& e : sx::g_prof_entries) {
        sx::g_prof_pool.push_back(e.start);
        sx::g_prof_pool.push_back(e.stop);
    }
    sx::g_prof_entries.clear();
    return SX_OK;
}

}  // extern "C"
