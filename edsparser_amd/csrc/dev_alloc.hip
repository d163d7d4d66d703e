// dev_alloc.hip — where every DevBuf gets its memory: the only hipMalloc / hipFree of the library.
//
// The product definitions (first half) are what DevBuf::ensure / release did inline.  With -DEDSX_GUARD the file defines
// the guard variant instead, linked into libedsx_guard.so for the tests only (tests/test_guard_gpu.py):
// every allocation is [front zone | payload | back zone], all three filled with one byte value, and the zones are looked at
// after each call.  Plain HIP: no kernel is instrumented and every access it watches for lands in memory the process owns.
#include "msa_device.hpp"

#ifndef EDSX_GUARD

namespace edsx {

void dev_alloc(size_t bytes, void** ptr, size_t* cap)
{
    if (*ptr) { (void)hipFree(*ptr); *ptr = nullptr; *cap = 0; }
    size_t want = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(ptr, want);
    if (e != hipSuccess) {
        *ptr = nullptr;
        (void)hipGetLastError();                              // (the failure is reported here, not by the next launch check)
        const std::string what = std::string("hipMalloc of ") + std::to_string(want) + " bytes: " + hipGetErrorString(e);
        if (e == hipErrorOutOfMemory) throw OutOfDeviceMemory(what);
        throw DeviceError(what);
    }
    *cap = want;
}

void dev_free(void* ptr) { (void)hipFree(ptr); }

} // namespace edsx

#else // EDSX_GUARD

#include <cstdio>
#include <dlfcn.h>
#include <execinfo.h>
#include <map>
#include <memory>

namespace edsx {
namespace {

constexpr size_t ZONE = 64 << 10;        // bytes in front of and behind every payload (a multiple of 256: the payload stays aligned)
constexpr int DEFAULT_FILL = 0x0A;       // '\n': a byte every text parser of the library reacts to

struct Live {
    uint8_t* base;       // what hipMalloc returned: front zone, payload at base + ZONE, back zone at base + ZONE + bytes
    size_t bytes;        // as requested (not rounded)
    u64 serial;
    int fill, dev;
};

struct Violation {
    u64 serial; size_t bytes; bool back, at_free; long long first, last; int fill; unsigned n; uint8_t found[16];
};

struct Registry {
    std::mutex mu;
    std::map<void*, Live> live;          // by payload address
    std::vector<Violation> seen;         // since the last check
    u64 serial = 0, allocs = 0, guarded = 0, checks = 0, unreadable = 0;
    int fill = DEFAULT_FILL;
    bool trace = false;
    std::vector<uint8_t> host = std::vector<uint8_t>(ZONE);
};

Registry& reg()
{
    static Registry* r = [] {
        Registry* x = new Registry;      // never destroyed: DevBufs of static objects are released after main
        const char* t = std::getenv("EDSX_GUARD_TRACE");
        x->trace = t && *t && *t != '0';
        return x;
    }();
    return *r;
}

// one zone of one allocation: download, compare, record and repair (so that a dirtied zone is reported once).  mu is held.
void sweep_zone(Registry& r, const Live& a, bool back, bool at_free)
{
    uint8_t* zone = back ? a.base + ZONE + a.bytes : a.base;
    if (hipMemcpy(r.host.data(), zone, ZONE, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();         // (process teardown: the runtime is gone before the last static DevBuf)
        r.unreadable++;
        return;
    }
    const uint8_t* h = r.host.data();
    size_t lo = 0, hi = ZONE;
    while (lo < ZONE && h[lo] == (uint8_t)a.fill) lo++;
    if (lo == ZONE) return;
    while (h[hi - 1] == (uint8_t)a.fill) hi--;
    Violation v{};
    v.serial = a.serial; v.bytes = a.bytes; v.back = back; v.at_free = at_free; v.fill = a.fill;
    // offsets relative to the payload edge: the back zone starts at +0, the front zone ends at -1
    v.first = back ? (long long)lo : (long long)lo - (long long)ZONE;
    v.last = back ? (long long)hi - 1 : (long long)hi - 1 - (long long)ZONE;
    for (size_t i = lo; i < hi && v.n < sizeof v.found; i++)
        if (h[i] != (uint8_t)a.fill) v.found[v.n++] = h[i];
    r.seen.push_back(v);
    if (!at_free) {
        (void)hipMemset(zone + lo, a.fill, hi - lo);
        (void)hipDeviceSynchronize();
    }
}

void sweep(Registry& r, const Live& a, bool at_free)
{
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != a.dev) (void)hipSetDevice(a.dev);
    (void)hipDeviceSynchronize();        // kernels in flight finish first (hipFree implies the same in the product build)
    sweep_zone(r, a, false, at_free);
    sweep_zone(r, a, true, at_free);
    if (cur != a.dev) (void)hipSetDevice(cur);
}

void release_locked(Registry& r, void* payload)
{
    auto it = r.live.find(payload);
    if (it == r.live.end()) { (void)hipFree(payload); return; }      // (not ours: cannot happen, every DevBuf comes from dev_alloc)
    sweep(r, it->second, true);
    (void)hipFree(it->second.base);
    r.live.erase(it);
}

__attribute__((noinline)) void trace_alloc(const Live& a)
{
    // the return addresses above dev_alloc as offsets into the library (DevBuf::ensure is usually inlined, so the first one
    // is already the ensure call site; `addr2line -e libedsx_guard.so 0x...` or the symbol table name it)
    void* bt[5];
    const int n = backtrace(bt, 5);
    char line[256];
    int at = std::snprintf(line, sizeof line, "edsx-guard: alloc #%llu %zu bytes from", (unsigned long long)a.serial, a.bytes);
    for (int i = 2; i < n && at < (int)sizeof line - 40; i++) {
        Dl_info di{};
        if (dladdr(bt[i], &di) && di.dli_fbase) {
            const char* slash = di.dli_fname ? std::strrchr(di.dli_fname, '/') : nullptr;
            at += std::snprintf(line + at, sizeof line - at, " %s+0x%zx", slash ? slash + 1 : "?", (size_t)((char*)bt[i] - (char*)di.dli_fbase));
        } else
            at += std::snprintf(line + at, sizeof line - at, " %p", bt[i]);
    }
    std::fprintf(stderr, "%s\n", line);
}

__global__ void k_guard_selftest_store(uint8_t* payload, const long long* off, int k)
{
    if (blockIdx.x == 0 && (int)threadIdx.x < k) payload[off[threadIdx.x]] = 0xA5 ^ (uint8_t)threadIdx.x;
}

} // namespace

void dev_alloc(size_t bytes, void** ptr, size_t* cap)
{
    Registry& r = reg();
    std::lock_guard<std::mutex> lock(r.mu);
    if (*ptr) { release_locked(r, *ptr); *ptr = nullptr; *cap = 0; }
    const size_t want = ZONE + ((bytes + 255) & ~(size_t)255) + ZONE;       // (the back zone is ZONE bytes from payload + bytes: it fits)
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, want);
    if (e == hipSuccess) {
        e = hipMemset(base, r.fill, want);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) (void)hipFree(base);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const std::string what = std::string("hipMalloc of ") + std::to_string(want) + " bytes: " + hipGetErrorString(e);
        if (e == hipErrorOutOfMemory) throw OutOfDeviceMemory(what);
        throw DeviceError(what);
    }
    Live a{static_cast<uint8_t*>(base), bytes, ++r.serial, r.fill, 0};
    (void)hipGetDevice(&a.dev);
    r.allocs++;
    r.guarded += bytes;
    *ptr = a.base + ZONE;
    *cap = bytes;                        // not rounded: a request for one byte more reallocates, and the back zone starts at the first byte nobody asked for
    r.live[*ptr] = a;
    if (r.trace) trace_alloc(a);
}

void dev_free(void* ptr)
{
    Registry& r = reg();
    std::lock_guard<std::mutex> lock(r.mu);
    release_locked(r, ptr);
}

} // namespace edsx

// ---- exported by libedsx_guard.so only (not in include/edsx.h) ------------------------------------------------------------
extern "C" {

// The byte every later allocation is filled with (zones and payload).  Default 0x0A.
void edsx_guard_set_fill(int byte)
{
    edsx::Registry& r = edsx::reg();
    std::lock_guard<std::mutex> lock(r.mu);
    r.fill = byte & 0xff;
}

// Sweeps the zones of all live allocations; returns the number of zones found dirty since the last check, those of buffers
// freed or regrown in between included.  text (cap bytes, may be null) gets one line per zone, the first one first:
//   "#<serial> <bytes> bytes, <front|back> zone, offsets <first>..<last>, fill <xx>, found <xx xx ..>[, at free]"
// Offsets are relative to the payload's edge: +0 is the first byte behind it, -1 the last byte in front of it.
uint64_t edsx_guard_check(char* text, size_t cap)
{
    edsx::Registry& r = edsx::reg();
    std::lock_guard<std::mutex> lock(r.mu);
    r.checks++;
    for (auto& kv : r.live) edsx::sweep(r, kv.second, false);
    size_t at = 0;
    if (text && cap) text[0] = 0;
    for (const edsx::Violation& v : r.seen) {
        if (!text || at + 200 > cap) break;
        at += std::snprintf(text + at, cap - at, "#%llu %zu bytes, %s zone, offsets %+lld..%+lld, fill %02x, found", (unsigned long long)v.serial,
                            v.bytes, v.back ? "back" : "front", v.first, v.last, v.fill);
        for (unsigned i = 0; i < v.n; i++) at += std::snprintf(text + at, cap - at, " %02x", v.found[i]);
        at += std::snprintf(text + at, cap - at, "%s\n", v.at_free ? ", at free" : "");
    }
    const uint64_t n = r.seen.size();
    r.seen.clear();
    return n;
}

// out[0..4]: allocations made, payload bytes guarded, checks run, live allocations, zones that could not be read
void edsx_guard_counters(uint64_t* out)
{
    edsx::Registry& r = edsx::reg();
    std::lock_guard<std::mutex> lock(r.mu);
    out[0] = r.allocs; out[1] = r.guarded; out[2] = r.checks; out[3] = r.live.size(); out[4] = r.unreadable;
}

// Self-test of the checker: a DevBuf of n bytes, then one kernel that stores a byte at each of the k payload offsets
// (-65536 <= offset < n + 65536: inside the allocation, nothing can fault).  keep != 0 holds the buffer until the next
// call (n == 0 only releases it), so that edsx_guard_check finds it live; otherwise it is freed before the call returns
// and the stores are found on its way out.  Returns the number of payload bytes that did not hold the fill before the
// stores (0), or -1 for arguments out of range or a HIP error.
long long edsx_guard_selftest(uint64_t n, const long long* offsets, int k, int keep)
{
    static std::unique_ptr<edsx::DevBuf> kept;
    kept.reset();
    if (n == 0) return 0;
    if (k < 0 || k > 64) return -1;
    for (int i = 0; i < k; i++)
        if (offsets[i] < -(long long)edsx::ZONE || offsets[i] >= (long long)(n + edsx::ZONE)) return -1;
    try {
        std::unique_ptr<edsx::DevBuf> b(new edsx::DevBuf), off(new edsx::DevBuf);
        int fill;
        { edsx::Registry& r = edsx::reg(); std::lock_guard<std::mutex> lock(r.mu); fill = r.fill; }
        b->ensure(n);
        if (b->cap != n || ((uintptr_t)b->ptr & 255)) return -1;
        std::vector<uint8_t> h(n);
        EDSX_HIP(hipMemcpy(h.data(), b->ptr, n, hipMemcpyDeviceToHost));
        long long bad = 0;
        for (uint8_t x : h) bad += x != (uint8_t)fill;
        if (k) {
            off->ensure(8 * (size_t)k);
            EDSX_HIP(hipMemcpy(off->ptr, offsets, 8 * (size_t)k, hipMemcpyHostToDevice));
            edsx::k_guard_selftest_store<<<1, 64>>>(b->as<uint8_t>(), off->as<long long>(), k);
            EDSX_HIP(hipGetLastError());
            EDSX_HIP(hipDeviceSynchronize());
        }
        if (keep) kept = std::move(b);
        return bad;
    } catch (const std::exception&) {
        return -1;
    }
}

} // extern "C"

#endif // EDSX_GUARD
