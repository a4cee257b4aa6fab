// Process-wide seams of the library (host only, no kernels): kernel-form log, kernel-form switch table, named-kernel timing.  Their
// hot side is inline in common.h, the control side is declared in conv.h (test entry points: include/dyffusion_hip_testing.h).
#include "conv.h"

#include <deque>
#include <map>
#include <mutex>
#include <string>

// ---- kernel-form log (common.h): form name + "@rows" -> launches noted since it was enabled
bool g_dyf_form_log_on = false;
static std::mutex g_form_mu;
static std::map<std::string, long long> g_form_log;
void dyf_form_note_slow(const char* form, long long rows) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    ++g_form_log[std::string(form) + "@" + std::to_string(rows)];
}
void dyf_form_log_enable(bool on) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    g_form_log.clear();
    g_dyf_form_log_on = on;
}
std::string dyf_form_log_text() {
    std::lock_guard<std::mutex> lk(g_form_mu);
    std::string t;
    for (auto& kv : g_form_log) t += kv.first + "=" + std::to_string(kv.second) + ";";
    return t;
}
// ---- kernel-form switches (common.h dyf_form): key -> value, set only through dyf_debug_set_form.  Values are interned and never
// freed (a pointer handed out by dyf_form stays valid for the life of the process).
int g_dyf_form_count = 0;
static std::map<std::string, const char*> g_form_values;
static std::deque<std::string> g_form_arena;
const char* dyf_form_slow(const char* key) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    auto it = g_form_values.find(key);
    return it == g_form_values.end() ? nullptr : it->second;
}
void dyf_form_set(const char* key, const char* value) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    if (!key) g_form_values.clear();
    else if (!value) g_form_values.erase(key);
    else {
        g_form_arena.emplace_back(value);
        g_form_values[key] = g_form_arena.back().c_str();
    }
    __atomic_store_n(&g_dyf_form_count, (int)g_form_values.size(), __ATOMIC_RELEASE);
}
std::string dyf_form_text() {
    std::lock_guard<std::mutex> lk(g_form_mu);
    std::string t;
    for (auto& kv : g_form_values) t += kv.first + "=" + kv.second + ";";
    return t;
}
// ---- named-kernel timing (common.h KernelProf): (start, stop, algorithmic bytes) of every launch of the armed name
const char* g_dyf_prof_name = nullptr;
static std::string g_prof_name_store;
struct ProfRec { hipEvent_t e0, e1; double bytes; };
static std::deque<ProfRec> g_prof_recs;
void dyf_prof_begin(hipStream_t st, double bytes) {
    std::lock_guard<std::mutex> lk(g_form_mu);  // (records of concurrent host threads interleave but stay whole; ONE armed name per process)
    ProfRec r{nullptr, nullptr, bytes};
    if (g_prof_recs.size() >= 16384 || hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
    (void)hipEventRecord(r.e0, st);
    g_prof_recs.push_back(r);
}
void dyf_prof_end(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    if (!g_prof_recs.empty()) (void)hipEventRecord(g_prof_recs.back().e1, st);
}
static void prof_arm_locked(const char* name) {
    for (auto& r : g_prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_prof_recs.clear();
    g_prof_name_store = name ? name : "";
    g_dyf_prof_name = name ? g_prof_name_store.c_str() : nullptr;
}
void dyf_prof_arm(const char* name) {  // nullptr disarms; pending records are dropped
    std::lock_guard<std::mutex> lk(g_form_mu);
    prof_arm_locked(name);
}
// after the stream has been synchronised: total ms, total bytes, launches of the armed name; disarms
void dyf_prof_collect(double* total_ms, double* total_bytes, int* launches) {
    std::lock_guard<std::mutex> lk(g_form_mu);
    double ms = 0.0, by = 0.0;
    int n = 0;
    for (auto& r : g_prof_recs) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) { ms += t; by += r.bytes; ++n; }
    }
    *total_ms = ms; *total_bytes = by; *launches = n;
    prof_arm_locked(nullptr);
}
