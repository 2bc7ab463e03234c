// Error reporting and device queries of libstk.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "stk_common.h"

static thread_local char g_err[1024] = "";

void stk_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *stk_last_error(void) { return g_err; }

extern "C" int stk_version(void) { return 200; }

// ---- the seam of dev_arrays.h: every plan's device arrays come and go through here ----
void *stk_dev_malloc(size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) return p;
    stk_set_error("hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return nullptr;
}

void stk_dev_free(void *p) { (void)hipFree(p); }

bool stk_dev_copy_in(void *dst, const void *src, size_t bytes)
{
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) stk_set_error("hipMemcpy of %zu bytes to the device failed: %s", bytes, hipGetErrorString(e));
    return e == hipSuccess;
}

// ---- tuning keys (stk.h documents each one) ------------------------------------
stk_tuning g_tuning;

namespace {

enum TuneKind { TUNE_LAUNCH, TUNE_PLAN, TUNE_COUNTER };

struct TuneKey {
    const char *name;
    std::atomic<int32_t> stk_tuning::*field;
    int32_t lo, hi;  // accepted values
    TuneKind kind;   // read at every launch / when a plan is created / a counter (0 resets, n > 0 checks)
};

const TuneKey k_tune_keys[] = {
    {"ell_wg_per_cu", &stk_tuning::ell_wg_per_cu, 0, 16, TUNE_LAUNCH},
    {"ell_force_wide", &stk_tuning::ell_force_wide, 0, 1, TUNE_LAUNCH},
    {"rows_force_wide", &stk_tuning::rows_force_wide, 0, 1, TUNE_LAUNCH},
    {"pack_rows", &stk_tuning::pack_rows, 1, 2, TUNE_PLAN},
    {"pack_multi_lanes", &stk_tuning::pack_multi_lanes, 0, 2, TUNE_LAUNCH},
    {"pack_check_steps", &stk_tuning::pack_check_steps, 0, 1, TUNE_LAUNCH},
    {"mg_strip_mb", &stk_tuning::mg_strip_mb, 0, 1 << 20, TUNE_LAUNCH},
    {"mg_strip_width", &stk_tuning::mg_strip_width, 0, 1 << 10, TUNE_LAUNCH},
    {"mg_strips_used", &stk_tuning::mg_strips_used, 0, INT32_MAX, TUNE_COUNTER},
    {"mg_zero_start", &stk_tuning::mg_zero_start, 0, 1, TUNE_LAUNCH},
    {"mg_gs_diag_free", &stk_tuning::mg_gs_diag_free, 0, 2, TUNE_PLAN},
    {"mg_fuse_restrict", &stk_tuning::mg_fuse_restrict, 0, 1, TUNE_LAUNCH},
    {"mg_restrict_one_pass", &stk_tuning::mg_restrict_one_pass, 0, 2, TUNE_LAUNCH},
    {"mg_fuse_coarse", &stk_tuning::mg_fuse_coarse, 0, 1, TUNE_LAUNCH},
    {"mg_coarse_lds", &stk_tuning::mg_coarse_lds, 0, 1, TUNE_LAUNCH},
    {"mg_coarse_uniform", &stk_tuning::mg_coarse_uniform, 0, 2, TUNE_LAUNCH},
};

}  // namespace

extern "C" int stk_set_tuning(const char *key, int32_t value)
{
    STK_REQUIRE(key != nullptr, "stk_set_tuning: null key");
    for (const TuneKey &k : k_tune_keys) {
        if (std::strcmp(key, k.name) != 0) continue;
        STK_REQUIRE(value >= k.lo && value <= k.hi, "stk_set_tuning: %s=%d not in %d..%d", k.name, value, k.lo, k.hi);
        std::atomic<int32_t> &v = g_tuning.*k.field;
        if (k.kind == TUNE_COUNTER && value > 0) {
            const int32_t n = v.load(std::memory_order_relaxed);
            STK_REQUIRE(n >= value, "stk_set_tuning: %s: %d so far, %d required", k.name, n, value);
            return 0;
        }
        v.store(value, std::memory_order_relaxed);
        return 0;
    }
    stk_set_error("stk_set_tuning: unknown key '%s'", key);
    return 2;
}

int stk_cu_count()
{
    // per device (one process may drive several), queried once per device and thread
    static thread_local int cached[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cached[dev] = n;
        else
            cached[dev] = 256;
    }
    return cached[dev];
}

extern "C" int stk_device_info(int32_t *n_cu, int32_t *wave_size, int64_t *hbm_bytes)
{
    int dev = 0;
    STK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    STK_HIP(hipGetDeviceProperties(&p, dev));
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (wave_size) *wave_size = p.warpSize;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return 0;
}

// ---- per-operation device-time counters ----------------------------------------
bool g_stk_timing = false;

namespace {

struct Bracket {
    hipEvent_t begin, end;
    int op;
};
std::mutex g_timing_mutex;
std::vector<Bracket *> g_timing_open, g_timing_spare;  // recorded, not yet read / reusable
double g_timing_seconds[STK_OP_CLASSES] = {0};
int64_t g_timing_calls[STK_OP_CLASSES] = {0};
const char *const g_timing_names[STK_OP_CLASSES] = {"kron", "space", "time", "wavelet", "multigrid", "blas1"};

// reads every recorded bracket (waits for its end event); caller holds the mutex
void timing_collect()
{
    for (Bracket *b : g_timing_open) {
        float ms = 0.0f;
        if (hipEventSynchronize(b->end) == hipSuccess && hipEventElapsedTime(&ms, b->begin, b->end) == hipSuccess) {
            g_timing_seconds[b->op] += 1.0e-3 * ms;
            g_timing_calls[b->op] += 1;
        }
        g_timing_spare.push_back(b);
    }
    g_timing_open.clear();
}

}  // namespace

void *stk_timing_begin(int op, hipStream_t st)
{
    Bracket *b = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_timing_mutex);
        if (!g_timing_spare.empty()) {
            b = g_timing_spare.back();
            g_timing_spare.pop_back();
        }
    }
    if (!b) {
        b = new Bracket();
        if (hipEventCreate(&b->begin) != hipSuccess || hipEventCreate(&b->end) != hipSuccess) {
            delete b;
            return nullptr;
        }
    }
    b->op = op;
    (void)hipEventRecord(b->begin, st);
    return b;
}

void stk_timing_end(void *slot, hipStream_t st)
{
    Bracket *b = static_cast<Bracket *>(slot);
    (void)hipEventRecord(b->end, st);
    std::lock_guard<std::mutex> lock(g_timing_mutex);
    g_timing_open.push_back(b);
    if (g_timing_open.size() >= 4096) timing_collect();  // bounded number of live events
}

extern "C" int stk_timing_enable(int32_t on)
{
    g_stk_timing = on != 0;
    return 0;
}

extern "C" int stk_timing_reset(void)
{
    std::lock_guard<std::mutex> lock(g_timing_mutex);
    timing_collect();
    for (int c = 0; c < STK_OP_CLASSES; ++c) g_timing_seconds[c] = 0.0, g_timing_calls[c] = 0;
    return 0;
}

extern "C" int stk_timing_get(const char *op_class, int64_t *calls, double *seconds)
{
    STK_REQUIRE(op_class != nullptr, "stk_timing_get: null class name");
    std::lock_guard<std::mutex> lock(g_timing_mutex);
    timing_collect();
    for (int c = 0; c < STK_OP_CLASSES; ++c)
        if (std::strcmp(op_class, g_timing_names[c]) == 0) {
            if (calls) *calls = g_timing_calls[c];
            if (seconds) *seconds = g_timing_seconds[c];
            return 0;
        }
    stk_set_error("stk_timing_get: unknown class '%s' (kron, space, time, wavelet, multigrid, blas1)", op_class);
    return 2;
}
