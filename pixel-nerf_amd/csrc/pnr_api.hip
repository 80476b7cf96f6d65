// pnr_api.hip -- error plumbing and library facts for libpixelnerf_hip.so.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

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

// ---- fp16-range guard of the fp32-class ("f16x3") kernels
static thread_local unsigned int *g_sat_flags = nullptr;
static thread_local int g_sat_slot = 0;

unsigned int *pnr::saturation_guard_word() { return g_sat_flags ? g_sat_flags + g_sat_slot : nullptr; }
void pnr::saturation_guard_slot(int slot) { g_sat_slot = slot == 1 ? 1 : 0; }

extern "C" int pnr_saturation_guard(unsigned int *flags_dev) {
    g_sat_flags = flags_dev;
    g_sat_slot = 0;
    return PNR_OK;
}

// ---- range probe of the same kernels: armed per host thread, slotted with the guard (saturation_guard_slot)
static thread_local float *g_probe = nullptr;

float *pnr::range_probe_words() { return g_probe ? g_probe + g_sat_slot * pnr::PROBE_WORDS : nullptr; }

extern "C" int pnr_range_probe(float *amax_dev) {
    g_probe = amax_dev;
    g_sat_slot = 0;
    return PNR_OK;
}

// ---- which split-operand blobs were packed at a stream scale.  The scale lives in the blob's tail (device memory); the host
// picks the kernel instantiation, so pnr_pack_mlp_split notes the ADDRESS it packed at s > 0 here (and forgets it when the same
// address is packed at 0).  A fixed table, no allocation; blobs at s = 0 -- every blob before revision 11 -- never enter it and
// their launches pay one relaxed load.
namespace {
struct ScaledBlob { const void *p; int s; };
constexpr int kMaxScaled = 256;
ScaledBlob g_scaled[kMaxScaled];
std::atomic<int> g_n_scaled{0};
std::mutex g_scaled_mu;
}  // namespace

int pnr::note_stream_scale(const void *packed, int s) {
    std::lock_guard<std::mutex> lock(g_scaled_mu);
    int n = g_n_scaled.load(std::memory_order_relaxed);
    for (int i = 0; i < n; ++i)
        if (g_scaled[i].p == packed) {
            if (s > 0) g_scaled[i].s = s;
            else { g_scaled[i] = g_scaled[n - 1]; g_n_scaled.store(n - 1, std::memory_order_release); }
            return PNR_OK;
        }
    if (s <= 0) return PNR_OK;
    if (n == kMaxScaled) return pnr_fail(PNR_E_INVALID, "pnr_pack_mlp_split: more than 256 live blobs packed at a stream scale");
    g_scaled[n] = {packed, s};
    g_n_scaled.store(n + 1, std::memory_order_release);
    return PNR_OK;
}

int pnr::stream_scale_of(const void *packed) {
    if (g_n_scaled.load(std::memory_order_acquire) == 0) return 0;
    std::lock_guard<std::mutex> lock(g_scaled_mu);
    const int n = g_n_scaled.load(std::memory_order_relaxed);
    for (int i = 0; i < n; ++i)
        if (g_scaled[i].p == packed) return g_scaled[i].s;
    return 0;
}
