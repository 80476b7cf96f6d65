// pnr_api.hip -- error plumbing and library facts for libpixelnerf_hip.so.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pnr_common.h"
#include "pnr_internal.h"
#include "pnr_layout.h"

static thread_local char g_err[512] = "";

int pnr_fail(int code, const char *msg) {
    std::snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "");
    return code;
}

int pnr_check_hip(hipError_t e, const char *where) {
    if (e == hipSuccess) return PNR_OK;
    std::snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return PNR_E_HIP;
}

int pnr_check_launch(const char *where) { return pnr_check_hip(hipGetLastError(), where); }

extern "C" const char *pnr_last_error(void) { return g_err; }

extern "C" int pnr_version(int *major, int *minor) {
    if (major) *major = 0;
    if (minor) *minor = 1;
    return PNR_OK;
}

// A library built with experiment switches (tools/build_variant.sh passes -DPNR_VARIANT next to them; the kernel sources only
// honour a switch under `#if defined(PNR_VARIANT) && defined(...)`) identifies itself with a NEGATIVE revision: the product
// binding refuses it (pixelnerf_amd/_lib.py), the A/B tools opt in.
extern "C" int pnr_abi_version(void) {
#ifdef PNR_VARIANT
    return -PNR_ABI_VERSION;
#else
    return PNR_ABI_VERSION;
#endif
}

extern "C" int pnr_device_info(int *num_cus, int *lds_bytes_per_block) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return pnr_check_hip(e, "hipGetDevice");
    if (num_cus) *num_cus = pnr::device_cus();
    if (lds_bytes_per_block) *lds_bytes_per_block = pnr::LDS_TOTAL;
    return PNR_OK;
}

// the multi-view kernels park one tile of fp32 view sums per workgroup; 96 points is the largest tile (the f16 training forward)
extern "C" size_t pnr_mv_workspace_bytes(void) { return (size_t)pnr::device_cus() * 96 * pnr::D_HID * sizeof(float); }

// a fact of the current device, queried once per device ordinal (0 = not asked yet: threads that race store the same value)
static int per_device(std::atomic<int> *cache, int (*query)(int dev), int fallback) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fallback;
    int n = cache[dev].load(std::memory_order_relaxed);
    if (!n) {
        n = query(dev);
        cache[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int pnr::device_xcd_count() {
    // the override is read per call (a getenv, no device work): tests switch the tile order inside one process
    if (const char *ov = std::getenv("PIXELNERF_XCD_COUNT")) {
        const int n = std::atoi(ov);
        return n > 0 ? n : 0;
    }
    static std::atomic<int> cache[64];
    return per_device(cache, [](int dev) {
        int n = 0;
        return hipDeviceGetAttribute(&n, hipDeviceAttributeNumberOfXccs, dev) == hipSuccess && n > 0 ? n : 1;
    }, 0);
}

int pnr::device_cus() {
    static std::atomic<int> cache[64];
    return per_device(cache, [](int dev) {
        int n = 0;
        return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }, 256);
}
