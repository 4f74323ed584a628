// The HIP host layer under the BAM-side stages (hotspots.hip, candidates.hip, refblocks.hip, phase.hip, haplotag.hip, markdup.hip): opening the device,
// owned device memory, the upload of a read set, timing a launch, the tail of an entry point, and what a handle that takes a
// chromosome span after span keeps (SpanHandle, CountTable).  No kernel lives here.
#pragma once
#include <utility>

#include <hip/hip_runtime.h>

#include "cigar.h"

namespace hello {
int set_last_error(int code, const char* fmt, ...);      // engine.hip
int exception_status(const char* where) noexcept;         // engine.hip

namespace {

#define HS_HIP(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) raise(HELLO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
    } while (0)

// The tail of every entry point that can refuse or allocate: `int hello_x(...) try { ... } HS_ENTRY_END("hello_x")`.
#define HS_ENTRY_END(name)                                                                                 \
    catch (const hello::Fail& f) { return hello::set_last_error(f.code, "%s", f.msg.c_str()); }            \
    catch (...) { return hello::exception_status(name); }

void open_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) raise(HELLO_ERR_NOGPU, "no GPU visible");
    if (device < 0 || device >= n_dev) raise(HELLO_ERR_ARG, "device %d of %d", device, n_dev);
    hipDeviceProp_t prop;
    HS_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        raise(HELLO_ERR_NOGPU, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    HS_HIP(hipSetDevice(device));
}

struct DevMem {
    std::vector<void*> ptrs;
    template <class T> T* put(const T* src, size_t n) {
        void* p = nullptr;
        HS_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(p);
        if (n) HS_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return (T*)p;
    }
    template <class T> T* room(size_t n) {                         // not initialised: for what a kernel writes in full
        void* p = nullptr;
        HS_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(p);
        return (T*)p;
    }
    template <class T> T* zeros(size_t n) {
        void* p = nullptr;
        HS_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(p);
        HS_HIP(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
        return (T*)p;
    }
    template <class T> T* release(T* p) {                          // p leaves: a longer-lived owner frees it
        ptrs.erase(std::find(ptrs.begin(), ptrs.end(), (void*)p));
        return p;
    }
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
};

struct DeviceReads {
    const uint8_t* bases = nullptr; const uint8_t* quals = nullptr; const int64_t* read_off = nullptr;
    const uint32_t* cigars = nullptr; const int64_t* cigar_off = nullptr; const int64_t* ref_start = nullptr;
};

DeviceReads upload_reads(DevMem& m, const ReadsView& s) {
    const size_t n = (size_t)s.n, nb = n ? (size_t)s.read_off[n] : 0, nc = n ? (size_t)s.cigar_off[n] : 0;
    DeviceReads d;
    d.bases = m.put(s.bases, nb);
    d.quals = m.put(s.quals, nb);
    d.read_off = m.put(s.read_off, n + 1);
    d.cigars = m.put(s.cigars, nc);
    d.cigar_off = m.put(s.cigar_off, n + 1);
    d.ref_start = m.put(s.ref_start, n);
    return d;
}

struct KernelTimer {               // HIP events around a launch on the default stream; destroyed on every path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    KernelTimer() = default;
    void start() {
        if (!e0) HS_HIP(hipEventCreate(&e0));
        if (!e1) HS_HIP(hipEventCreate(&e1));
        HS_HIP(hipEventRecord(e0, 0));
    }
    float stop() {                 // after the launch: its error, if any, is the refusal
        float ms = 0.0f;
        HS_HIP(hipGetLastError());
        HS_HIP(hipEventRecord(e1, 0));
        HS_HIP(hipEventSynchronize(e1));
        HS_HIP(hipEventElapsedTime(&ms, e0, e1));
        return ms;
    }
    ~KernelTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    KernelTimer(const KernelTimer&) = delete;
    KernelTimer& operator=(const KernelTimer&) = delete;
};

// What a handle that takes a chromosome's reads span after span keeps (hello_meth, hello_pileup; hello_qc shares check_span).
inline void check_span(int64_t lo, int64_t hi, int64_t length, int64_t last_hi) {
    if (lo < 0 || hi <= lo || hi > length)
        raise(HELLO_ERR_ARG, "span [%lld, %lld) of a reference of %lld bases", (long long)lo, (long long)hi, (long long)length);
    if (lo < last_hi)
        raise(HELLO_ERR_ARG, "span [%lld, %lld) begins below %lld, where the previous one ended", (long long)lo, (long long)hi,
              (long long)last_hi);
}

template <int kStats> struct SpanHandle {
    int device = 0;
    int64_t length = 0, last_hi = 0, counting_given = 0;
    std::vector<uint8_t> status;                 // of the last add, per read
    double stats[kStats] = {0};
    void check_span(int64_t lo, int64_t hi) const { hello::check_span(lo, hi, length, last_hi); }
    // n more counting reads: refused past `cap`, which keeps the handle's 32-bit `what` from overflowing.  The add that has passed
    // all its checks commits them to counting_given itself.
    void take_counting(int64_t n, int64_t cap, const char* what) const {
        if (counting_given + n > cap)
            raise(HELLO_ERR_ARG, "more than %lld counting reads in one handle: its %s are 32-bit", (long long)cap, what);
    }
    int copy_stats(double* out) const {
        std::copy(stats, stats + kStats, out);
        return HELLO_OK;
    }
};

// A table of 32-bit counters the kernels add to, and its 64-bit copy on the host, fetched when asked for after a launch.
struct CountTable {
    DevMem mem;
    unsigned* device = nullptr;
    std::vector<int64_t> host;
    bool fetched = true;
    void build(size_t n) {                                         // zeros on both sides
        device = mem.zeros<unsigned>(n);
        host.assign(n, 0);
    }
    void swap(CountTable& o) {
        mem.ptrs.swap(o.mem.ptrs);
        std::swap(device, o.device);
        host.swap(o.host);
        std::swap(fetched, o.fetched);
    }
    const std::vector<int64_t>& fetch(int on_device) {
        if (!fetched) {
            HS_HIP(hipSetDevice(on_device));
            std::vector<unsigned> got(host.size());
            if (!got.empty()) HS_HIP(hipMemcpy(got.data(), device, got.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
            std::copy(got.begin(), got.end(), host.begin());
            fetched = true;
        }
        return host;
    }
};

struct PairHash {                                                // (name hash, strand): a read pair's two mates stay distinct
    size_t operator()(const std::pair<uint64_t, int>& k) const { return (size_t)(k.first * 0x9E3779B97F4A7C15ull) ^ (size_t)k.second; }
};

}  // namespace
}  // namespace hello
