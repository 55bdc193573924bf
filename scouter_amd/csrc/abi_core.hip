// ABI plumbing: version, thread-local error text, routing switches, dynamic-LDS limits, optional per-kernel-class hipEvent
// timing.
#include "common.h"

#include <stdarg.h>
#include <stdlib.h>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#define SCOUTER_ABI_VERSION 1

static thread_local char g_err[512] = "";
static thread_local hipError_t g_lds_err = hipSuccess;      // a failed sc_dyn_lds, for the next sc_check_launch

void sc_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int sc_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = g_lds_err;
    g_lds_err = hipSuccess;
    if (e != hipSuccess) {
        sc_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return SC_ERR_LAUNCH;
    }
    return SC_OK;
}

extern "C" int scouter_abi_version(void) { return SCOUTER_ABI_VERSION; }
extern "C" const char* scouter_last_error(void) { return g_err; }

// ---- routing switches (common.h ScSwitch): the only place the library reads the environment
static const char* const g_switch_names[SC_SW_COUNT] = {"xwt", "bwt", "bhalo", "xslot_small", "xslot_bwd_halves",
                                                         "xslot_bwd_scratch", "pwp_bn", "pwp_resident"};
struct SwitchTable {
    std::atomic<int> v[SC_SW_COUNT] = {};
    SwitchTable() {
        static const char* const flags[] = {"SCOUTER_XWT", "SCOUTER_BWT", "SCOUTER_BHALO", "SCOUTER_XSLOT_SMALL",
                                            "SCOUTER_XSLOT_BWD_HALVES", "SCOUTER_XSLOT_BWD_SCRATCH"};
        for (int i = 0; i <= SC_SW_XSLOT_BWD_SCRATCH; ++i) {      // a flag leaves its default only at a leading '0' / '1'
            const int def = i != SC_SW_XSLOT_BWD_SCRATCH;
            const char* e = getenv(flags[i]);
            v[i] = e && e[0] == '1' - def ? !def : def;
        }
        int bn = 0, r = 0;
        const char* e = getenv("SCOUTER_PWP_PLAN_DEV");         // "bn,resident"
        if (e && sscanf(e, "%d,%d", &bn, &r) == 2 && bn > 0 && r > 0) { v[SC_SW_PWP_BN] = bn; v[SC_SW_PWP_RESIDENT] = r; }
    }
};
static SwitchTable& switch_table() {
    static SwitchTable t;           // filled once, at first use (thread-safe)
    return t;
}
int sc_switch(ScSwitch s) { return switch_table().v[s].load(std::memory_order_relaxed); }

static int switch_index(const char* name) {
    for (int i = 0; name && i < SC_SW_COUNT; ++i)
        if (strcmp(name, g_switch_names[i]) == 0) return i;
    sc_set_error("unknown switch '%s'", name ? name : "(null)");
    return -1;
}
extern "C" int scouter_set_switch(const char* name, int value) {
    const int i = switch_index(name);
    if (i < 0) return SC_ERR_ARG;
    SC_REQUIRE(value >= 0, "switch '%s': negative value %d", name, value);
    switch_table().v[i].store(value, std::memory_order_relaxed);
    return SC_OK;
}
extern "C" int scouter_get_switch(const char* name) {
    const int i = switch_index(name);
    return i < 0 ? SC_ERR_ARG : sc_switch((ScSwitch)i);
}

// ---- dynamic LDS: the largest limit set so far per (kernel, device)
void sc_dyn_lds(const void* kern, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> limits;
    int dev = 0;
    hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = limits[{kern, dev}];
    if (bytes <= have) return;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    else g_lds_err = e;
}

// ---------------------------------------------------------------------------------------------------------------
// profiling: when enabled every launch of a kernel class is bracketed by two hipEvents on ITS stream
// ---------------------------------------------------------------------------------------------------------------
struct ProfRec { hipEvent_t a, b; const char* name; double flops, bytes; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;

ScProfScope::ScProfScope(const char* name, hipStream_t st, double flops, double bytes) : stream(st), slot(-1) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r;
    r.name = name; r.flops = flops; r.bytes = bytes;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    hipEventRecord(r.a, st);
    slot = (int)g_prof.size();
    g_prof.push_back(r);
}
ScProfScope::~ScProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEventRecord(g_prof[slot].b, stream);
}

extern "C" void scouter_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
}

// Synchronises the recorded events and writes one line per kernel name into `buf`:
//   name <tab> launches <tab> total_ms <tab> algorithmic_flops <tab> algorithmic_bytes \n
// then clears the log.  Returns the number of bytes written (truncated to cap-1), or -1 on a bad buffer.
extern "C" int scouter_prof_collect(char* buf, int cap) {
    if (!buf || cap <= 0) return -1;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    struct Agg { const char* name; double n, ms, fl, by; };
    std::vector<Agg> aggs;
    for (auto& r : g_prof) {
        float ms = 0.f;
        hipEventSynchronize(r.b);
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            Agg* a = nullptr;
            for (auto& x : aggs) if (strcmp(x.name, r.name) == 0) { a = &x; break; }
            if (!a) { aggs.push_back(Agg{r.name, 0, 0, 0, 0}); a = &aggs.back(); }
            a->n += 1; a->ms += ms; a->fl += r.flops; a->by += r.bytes;
        }
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
    }
    g_prof.clear();
    int off = 0;
    buf[0] = 0;
    for (auto& a : aggs) {
        int w = snprintf(buf + off, cap - off, "%s\t%.0f\t%.6f\t%.6e\t%.6e\n", a.name, a.n, a.ms, a.fl, a.by);
        if (w < 0 || w >= cap - off) break;
        off += w;
    }
    return off;
}
