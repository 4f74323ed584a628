// Read-backed phasing (include/hello_mi355x.h: hello_phase_*): aligned reads + the heterozygous records of one chromosome -> what
// every counted read shows at every record it spans (allele a, allele b or nothing), how often two records within a window were
// seen together in cis and in trans, and, once the host has chained the records into phase sets, a haplotype for every read.  Not
// in the reference; DESIGN.md section 7g states the rules and hello_amd/phase.py restates them in Python, integer for integer.
//
// Host: the read filter, the validation of every counted read (the kernel reads within its bases), per counted read its reference
// end from the CIGAR, the contiguous range of records whose start it covers (two binary searches in the sorted record starts) and,
// by an exclusive scan of those counts, the offset of its first slot.  Device, three kernels:
//   observe: a wave per counted read.  The lanes hold the read's candidate records, 64 per round; the walk over the CIGAR
//     (phase_walk.h, which haplotag.hip includes too) is wave-uniform
//     (one operation at a time, the same for all lanes, ended once every lane's record lies behind the cursor), and a
//     lane only has work where an operation meets its own span -- it compares the bases it would append with both alleles as it
//     goes, so no string is stored.  Each lane writes the slot of its own record: one writer per slot, no reduction across lanes.
//     (The opposite assignment -- lanes over the bases of an operation, a loop over the records -- puts 64 lanes on spans that are
//     one base long at most records and needs a cross-lane compare; section 7g.)
//   link: a thread per slot.  Slot distance within a read is record-index distance, so the thread looks back at most `window`
//     slots of its own read and adds 1 to link[t][k][cis | trans] in global memory with an integer atomic.
//   tag: a thread per counted read, one pass over its slots with the sets and flips the host chained.
// Slot capacity is exact, counters are integers and every slot and every tag has one writer: two runs give the same bytes.
//
// Fragments (hello_phase_fragments, hello_phase_tag_fragments): the two mates of a read pair act as one
// fragment.  After the last observe the handle's slots are joined into one device array and three more launches run over the
// counted reads of ALL batches, indexed c = 0..counted-1 in the order given:
//   pair (two kernels; they live in phase_pair.h, which markdup.hip includes too): an open-addressing table of 2^k >= 2 counted
//     slots in global memory.  Insert: a thread per counted read
//     claims the slot of its (name_hash, source) with atomicCAS on an int32 owner (-1 empty, else the claiming read) or finds the
//     slot whose owner has its key -- keys are compared in the input arrays, so no key value is reserved -- and counts itself
//     into the slot: reads, first mates, second mates, the smallest index of each kind (atomicAdd / atomicMin, the result does
//     not depend on arrival order; which read owns a slot does, and nothing reads the owner but the probe).  Look-up: a thread
//     per counted read finds its slot again and writes mate[c]; the slot's owner counts the group into pairs / groups_refused.
//   fragment link: a thread per slot.  Exactly one thread answers for a (fragment, record): the slot of the only read that
//     covers it or, where both mates do, the slot of the mate with the smaller index.  It evaluates F(t), looks back d = 1..window
//     and evaluates F(t - d) from at most two slot loads, one atomicAdd on int32 per link.
//   fragment tag: a thread per counted read, one pass over its range and its mate's in record order; both mates compute the same
//     answer and each writes its own.
#include <chrono>
#include <climits>
#include <memory>

#include "phase_pair.h"
#include "phase_walk.h"
#include "stage_host.h"

namespace hello {
namespace {

constexpr int kPhThreads = 256;
constexpr int kPhWaves = kPhThreads / 64;

struct PhObserveArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* list;         // the counted reads, in input order
    const int64_t* list_end;     // reference end of list[k], from its CIGAR
    const int64_t* first;        // [counted]: the first candidate record of list[k]
    const int64_t* slot_off;     // [counted + 1]: exclusive scan of the candidate counts
    const int64_t* rec_start;    // [records], sorted
    const int64_t* rec_end;
    const uint8_t* alleles;      // allele a then allele b of every record, upper case
    const int64_t* allele_off;   // [2 records + 1]
    int8_t* slots;
    int64_t n_counted;
    int q_threshold;
};

__global__ __launch_bounds__(kPhThreads) void phase_observe_kernel(PhObserveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * kPhWaves + (threadIdx.x >> 6);
    if (k >= a.n_counted) return;
    const int64_t s0 = a.slot_off[k], n_cand = a.slot_off[k + 1] - s0;
    if (n_cand == 0) return;
    const int64_t r = a.list[k], t0 = a.first[k], c0 = a.cigar_off[r];
    const PhWalkRead rd{a.bases + a.read_off[r], a.quals + a.read_off[r], a.cigars + c0, a.cigar_off[r + 1] - c0, a.ref_start[r],
                        a.list_end[k]};
    const PhWalkTable tb{a.rec_start, a.rec_end, a.alleles, a.allele_off};
    for (int64_t round = 0; round < n_cand; round += 64) {
        const int64_t j = round + lane;
        const bool mine = j < n_cand;
        const int o = phase_walk_observe(rd, tb, t0 + j, mine, a.q_threshold);     // every lane: the walk votes across the wave
        if (mine) a.slots[s0 + j] = (int8_t)o;
    }
}

struct PhLinkArgs {
    const int8_t* slots;
    const int64_t* slot_off;     // [counted + 1]
    const int64_t* first;
    int32_t* link;               // [records][window][2]
    int64_t n_slots, n_counted;
    int window;
};

__global__ __launch_bounds__(kPhThreads) void phase_link_kernel(PhLinkArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kPhThreads + threadIdx.x;
    if (s >= a.n_slots) return;
    const int o = a.slots[s];
    if (o < 0) return;
    int64_t x = 0, y = a.n_counted + 1;                                   // the last read whose first slot is at or before s
    while (x < y) {
        const int64_t mid = (x + y) >> 1;
        if (a.slot_off[mid] <= s) x = mid + 1; else y = mid;
    }
    const int64_t k = x - 1, base = a.slot_off[k], t = a.first[k] + (s - base);
    for (int d = 1; d <= a.window && s - d >= base; ++d) {
        const int p = a.slots[s - d];
        if (p < 0) continue;
        atomicAdd(&a.link[(t * a.window + (d - 1)) * 2 + (p != o ? 1 : 0)], 1);
    }
}

struct PhTagArgs {
    const int8_t* slots;
    const int64_t* slot_off;
    const int64_t* first;
    const int32_t* set;          // [records]: the record that opened the set
    const uint8_t* flip;
    const int64_t* set_pos;      // [records]: POS of the set's first record, 0 when the set has one member
    uint8_t* hp;                 // [counted]
    int64_t* ps;
    int64_t n_counted;
};

__global__ __launch_bounds__(kPhThreads) void phase_tag_kernel(PhTagArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kPhThreads + threadIdx.x;
    if (k >= a.n_counted) return;
    const int64_t s0 = a.slot_off[k], s1 = a.slot_off[k + 1], t0 = a.first[k];
    int mine = -1, n1 = 0, n2 = 0;
    int64_t pos = 0;
    for (int64_t s = s0; s < s1; ++s) {
        const int o = a.slots[s];
        const int64_t t = t0 + (s - s0);
        if (o < 0 || a.set_pos[t] == 0) continue;
        if (mine < 0) { mine = a.set[t]; pos = a.set_pos[t]; }
        if (a.set[t] != mine) continue;
        if ((o ^ (int)a.flip[t]) == 0) ++n1; else ++n2;
    }
    a.hp[k] = n1 > n2 ? 1 : n2 > n1 ? 2 : 0;
    a.ps[k] = pos;
}

// ---- fragments: links and tags -----------------------------------------------------------------------------------------------
struct PhFragArgs {
    const int8_t* slots;         // the batches' slots, joined
    const int64_t* slot_off;     // [counted + 1]
    const int64_t* first;        // [counted]
    const int32_t* mate;         // [counted]: the mate's counted index or -1
    int32_t* link;               // [records][window][2]
    int64_t n_slots, n_counted;
    int window;
    const int32_t* set;          // the tag launch: as PhTagArgs
    const uint8_t* flip;
    const int64_t* set_pos;
    uint8_t* hp;
    int64_t* ps;
};

struct PhRange { int64_t first, slot, n; };      // a read's candidate records [first, first + n) and its first slot

__device__ inline PhRange range_of(const PhFragArgs& a, int64_t k) {
    if (k < 0) return PhRange{0, 0, 0};
    const int64_t s = a.slot_off[k];
    return PhRange{a.first[k], s, a.slot_off[k + 1] - s};
}

__device__ inline bool covers(const PhRange& r, int64_t t) { return t >= r.first && t < r.first + r.n; }

// F(t) of the fragment whose reads have the ranges x and y: the value of the only slot that covers t; with two, the common
// value, the observed one where only one observed, none where they disagree.
__device__ inline int fragment_at(const int8_t* slots, const PhRange& x, const PhRange& y, int64_t t) {
    int o = -1;
    if (covers(x, t)) o = slots[x.slot + (t - x.first)];
    if (covers(y, t)) {
        const int p = slots[y.slot + (t - y.first)];
        if (o < 0) o = p;
        else if (p >= 0 && p != o) o = -1;
    }
    return o;
}

__global__ __launch_bounds__(kPhThreads) void phase_fragment_link_kernel(PhFragArgs a) {
    const int64_t s = (int64_t)blockIdx.x * kPhThreads + threadIdx.x;
    if (s >= a.n_slots) return;
    int64_t x = 0, y = a.n_counted + 1;                                   // the last read whose first slot is at or before s
    while (x < y) {
        const int64_t mid = (x + y) >> 1;
        if (a.slot_off[mid] <= s) x = mid + 1; else y = mid;
    }
    const int64_t k = x - 1, m = a.mate[k];
    const PhRange own = range_of(a, k), other = range_of(a, m);
    const int64_t t = own.first + (s - own.slot);
    if (m >= 0 && m < k && covers(other, t)) return;                      // the mate's slot answers for this record
    const int o = fragment_at(a.slots, own, other, t);
    if (o < 0) return;
    for (int d = 1; d <= a.window && t - d >= 0; ++d) {
        const int p = fragment_at(a.slots, own, other, t - d);
        if (p < 0) continue;
        atomicAdd(&a.link[(t * a.window + (d - 1)) * 2 + (p != o ? 1 : 0)], 1);
    }
}

__global__ __launch_bounds__(kPhThreads) void phase_fragment_tag_kernel(PhFragArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kPhThreads + threadIdx.x;
    if (k >= a.n_counted) return;
    PhRange lo = range_of(a, k), hi = range_of(a, a.mate[k]);
    if (lo.n == 0 || (hi.n > 0 && hi.first < lo.first)) { const PhRange z = lo; lo = hi; hi = z; }      // record order
    int mine = -1, n1 = 0, n2 = 0;
    int64_t pos = 0;
    const auto visit = [&](int64_t t) {
        const int o = fragment_at(a.slots, lo, hi, t);
        if (o < 0 || a.set_pos[t] == 0) return;
        if (mine < 0) { mine = a.set[t]; pos = a.set_pos[t]; }
        if (a.set[t] != mine) return;
        if ((o ^ (int)a.flip[t]) == 0) ++n1; else ++n2;
    };
    // lo's records, then what hi adds behind them: the records in a gap between the mates have no observation
    const int64_t end = lo.first + lo.n;
    for (int64_t t = lo.first; t < end; ++t) visit(t);
    if (hi.n > 0)
        for (int64_t t = hi.first > end ? hi.first : end; t < hi.first + hi.n; ++t) visit(t);
    a.hp[k] = n1 > n2 ? 1 : n2 > n1 ? 2 : 0;
    a.ps[k] = pos;
}

struct PhBatch {
    int8_t* slots = nullptr;     // device
    int64_t* slot_off = nullptr;
    int64_t* first = nullptr;
    int64_t n_counted = 0, n_slots = 0, read_base = 0;
    std::vector<int64_t> reads;  // list[k] of the batch
};

}  // namespace
}  // namespace hello

struct hello_phase {
    int device = 0, window = 0, q_threshold = 0, mapq_threshold = 0;
    int64_t n_records = 0, n_reads = 0;
    std::vector<int64_t> rec_start;
    int64_t* d_rec_start = nullptr;
    int64_t* d_rec_end = nullptr;
    uint8_t* d_alleles = nullptr;
    int64_t* d_allele_off = nullptr;
    std::vector<hello::PhBatch> batches;
    std::vector<int8_t> slots;
    std::vector<int64_t> slot_offsets{0}, first, ps;
    std::vector<int32_t> links;
    std::vector<uint8_t> hp;
    double stats[HELLO_PHASE_STATS] = {0};
    // fragments (hello_phase_fragments): the counted reads of all batches as one set, on the device until the handle goes
    bool fragments = false;
    int64_t n_counted = 0, n_slots = 0;
    std::vector<int64_t> counted_reads, mate;       // [counted]: the read of c in the order given; [reads]: the mate or -1
    std::vector<int32_t> fragment_links;
    int8_t* d_frag_slots = nullptr;
    int64_t* d_frag_slot_off = nullptr;
    int64_t* d_frag_first = nullptr;
    int32_t* d_frag_mate = nullptr;
    double fragment_stats[HELLO_PHASE_FRAGMENT_STATS] = {0};
    ~hello_phase() {
        for (auto& b : batches) { (void)hipFree(b.slots); (void)hipFree(b.slot_off); (void)hipFree(b.first); }
        (void)hipFree(d_frag_slots);
        (void)hipFree(d_frag_slot_off);
        (void)hipFree(d_frag_first);
        (void)hipFree(d_frag_mate);
        (void)hipFree(d_rec_start);
        (void)hipFree(d_rec_end);
        (void)hipFree(d_alleles);
        (void)hipFree(d_allele_off);
    }
};

namespace hello {
namespace {

// The chained set / flip a tag call is given, validated -> per record the POS of its set's first record, 0 for a set of one.
std::vector<int64_t> set_positions(const hello_phase* h, const int32_t* set, const uint8_t* flip) {
    const int64_t n = h->n_records;
    std::vector<int64_t> members((size_t)n, 0), set_pos((size_t)n, 0);
    for (int64_t t = 0; t < n; ++t) {
        if (set[t] < 0 || set[t] > t || set[set[t]] != set[t])
            raise(HELLO_ERR_ARG, "set[%lld] = %d: the record that opened the set, at or before it", (long long)t, set[t]);
        if (flip[t] > 1) raise(HELLO_ERR_ARG, "flip[%lld] = %d: 0 or 1", (long long)t, (int)flip[t]);
        ++members[set[t]];
    }
    for (int64_t t = 0; t < n; ++t) set_pos[t] = members[set[t]] >= 2 ? h->rec_start[set[t]] + 1 : 0;
    return set_pos;
}

}  // namespace
}  // namespace hello

extern "C" {

int hello_phase_observe(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                        const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                        const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                        const int64_t* record_starts, const int64_t* record_ends, const uint8_t* alleles,
                        const int64_t* allele_offsets, int64_t n_records, int32_t q_threshold, int32_t mapq_threshold,
                        int32_t window, int32_t device, hello_phase** handle) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!handle || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends ||
        !mapq || !flags || !name_hash || !source)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0 || n_records < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    hello_phase* h = *handle;
    std::unique_ptr<hello_phase> own;
    if (!h) {
        // ---- the first call of a chromosome: its records, validated and uploaded once
        if (!allele_offsets || (n_records > 0 && (!record_starts || !record_ends || !alleles)))
            return set_last_error(HELLO_ERR_ARG, "NULL pointer");
        if (window < 1 || window > HELLO_PHASE_MAX_WINDOW)
            return set_last_error(HELLO_ERR_ARG, "window %d: 1 to %d", window, HELLO_PHASE_MAX_WINDOW);
        if (n_records > INT32_MAX / (2 * HELLO_PHASE_MAX_WINDOW))
            return set_last_error(HELLO_ERR_ARG, "%lld records in one chromosome", (long long)n_records);
        if (allele_offsets[0] != 0) return set_last_error(HELLO_ERR_ARG, "allele_offsets[0] is not 0");
        for (int64_t t = 0; t < n_records; ++t) {
            if (record_starts[t] < 0 || record_ends[t] <= record_starts[t])
                return set_last_error(HELLO_ERR_ARG, "record %lld: span [%lld, %lld)", (long long)t, (long long)record_starts[t],
                                      (long long)record_ends[t]);
            if (t > 0 && record_starts[t] < record_starts[t - 1])
                return set_last_error(HELLO_ERR_ARG, "record %lld: records are not sorted by position", (long long)t);
            if (allele_offsets[2 * t + 1] < allele_offsets[2 * t] || allele_offsets[2 * t + 2] < allele_offsets[2 * t + 1])
                return set_last_error(HELLO_ERR_SHAPE, "record %lld: allele offsets decrease", (long long)t);
        }
        own.reset(new hello_phase());
        h = own.get();
        open_device(device);
        h->device = device;
        h->window = window;
        h->q_threshold = q_threshold;
        h->mapq_threshold = mapq_threshold;
        h->n_records = n_records;
        h->rec_start.assign(record_starts, record_starts + n_records);
        h->links.assign((size_t)n_records * window * 2, 0);
        DevMem m;                                                           // each upload leaves to the handle at once
        h->d_rec_start = m.release(m.put(record_starts, (size_t)n_records));
        h->d_rec_end = m.release(m.put(record_ends, (size_t)n_records));
        h->d_alleles = m.release(m.put(alleles, (size_t)allele_offsets[2 * n_records]));
        h->d_allele_off = m.release(m.put(allele_offsets, (size_t)(2 * n_records + 1)));
    } else {
        if (n_records != h->n_records || window != h->window || q_threshold != h->q_threshold || mapq_threshold != h->mapq_threshold ||
            device != h->device)
            return set_last_error(HELLO_ERR_ARG, "a further call names other records, thresholds, window or device than the first");
        HS_HIP(hipSetDevice(h->device));
    }
    if (!h->hp.empty() || !h->ps.empty()) return set_last_error(HELLO_ERR_ARG, "reads cannot be added after hello_phase_tag");
    if (h->fragments) return set_last_error(HELLO_ERR_ARG, "reads cannot be added after hello_phase_fragments");

    // ---- the counted reads, validated (the kernel reads within their bases), and the records each one's start-to-end covers
    const int64_t n = h->n_records;
    const int64_t* rec = h->rec_start.data();
    PhBatch b;
    struct Guard {                                                          // the batch's device memory, until the handle owns it
        PhBatch* b;
        ~Guard() {
            if (b) { (void)hipFree(b->slots); (void)hipFree(b->slot_off); (void)hipFree(b->first); }
        }
    } guard{&b};
    b.read_base = h->n_reads;
    std::vector<int64_t> list_end, first, slot_off{0}, all_first((size_t)n_reads, 0), all_count((size_t)n_reads, 0);
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    for (int64_t r = 0; r < n_reads; ++r) {
        if (source[r] > 1) return set_last_error(HELLO_ERR_ARG, "source[%lld] = %d: 0 or 1", (long long)r, (int)source[r]);
        int64_t qlen, rlen;
        if (!counted_walk(in, r, mapq_threshold, qlen, rlen)) continue;
        const int64_t end = ref_starts[r] + rlen;
        const int64_t f = std::lower_bound(rec, rec + n, ref_starts[r]) - rec;
        const int64_t l = std::lower_bound(rec, rec + n, end) - rec;
        const int64_t count = std::max<int64_t>(l - f, 0);
        b.reads.push_back(r);
        list_end.push_back(end);
        first.push_back(f);
        slot_off.push_back(slot_off.back() + count);                        // exclusive scan: the capacity is exact
        all_first[r] = f;
        all_count[r] = count;
    }
    b.n_counted = (int64_t)b.reads.size();
    b.n_slots = slot_off.back();
    const auto t1 = clock::now();

    float observe_ms = 0.0f, link_ms = 0.0f;
    std::vector<int8_t> slots((size_t)b.n_slots);
    if (b.n_slots > 0) {
        DevMem m;
        PhObserveArgs a{};
        const DeviceReads d = upload_reads(m, in);
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.list = m.put(b.reads.data(), b.reads.size());
        a.list_end = m.put(list_end.data(), list_end.size());
        b.first = m.release(m.put(first.data(), first.size()));
        b.slot_off = m.release(m.put(slot_off.data(), slot_off.size()));
        void* p = nullptr;
        HS_HIP(hipMalloc(&p, (size_t)b.n_slots));
        b.slots = (int8_t*)p;
        HS_HIP(hipMemset(p, 0xFF, (size_t)b.n_slots));
        const PhBatch& kept = b;
        a.first = kept.first;
        a.slot_off = kept.slot_off;
        a.rec_start = h->d_rec_start;
        a.rec_end = h->d_rec_end;
        a.alleles = h->d_alleles;
        a.allele_off = h->d_allele_off;
        a.slots = kept.slots;
        a.n_counted = b.n_counted;
        a.q_threshold = q_threshold;
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(phase_observe_kernel, dim3(blocks_for(b.n_counted, kPhWaves)), dim3(kPhThreads), 0, 0, a);
        observe_ms = timer.stop();
        PhLinkArgs l{};
        l.slots = kept.slots;
        l.slot_off = kept.slot_off;
        l.first = kept.first;
        l.link = m.zeros<int32_t>(h->links.size());
        l.n_slots = b.n_slots;
        l.n_counted = b.n_counted;
        l.window = h->window;
        timer.start();
        hipLaunchKernelGGL(phase_link_kernel, dim3(blocks_for(b.n_slots, kPhThreads)), dim3(kPhThreads), 0, 0, l);
        link_ms = timer.stop();
        HS_HIP(hipMemcpy(slots.data(), kept.slots, slots.size(), hipMemcpyDeviceToHost));
        std::vector<int32_t> link(h->links.size());
        HS_HIP(hipMemcpy(link.data(), l.link, link.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < link.size(); ++i) h->links[i] += link[i];    // the spans' links are added on the host
    }
    h->batches.push_back(b);                                                // without a slot: nothing on the device, the tags are 0
    guard.b = nullptr;
    // ---- the host's view, aligned with the reads given so far
    h->slots.insert(h->slots.end(), slots.begin(), slots.end());
    for (int64_t r = 0; r < n_reads; ++r) {
        h->first.push_back(all_first[r]);
        h->slot_offsets.push_back(h->slot_offsets.back() + all_count[r]);
    }
    h->n_reads += n_reads;
    h->stats[0] = (double)h->n_records;
    h->stats[1] = (double)h->n_reads;
    h->stats[2] += (double)b.n_counted;
    h->stats[3] += (double)b.n_slots;
    h->stats[4] += observe_ms;
    h->stats[5] += link_ms;
    h->stats[7] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->stats[8] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    if (own) *handle = own.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_phase_observe")

int hello_phase_chain(const int32_t* link, const int32_t* chromosome, int64_t n_records, int32_t window, int32_t min_margin,
                      int32_t* set, uint8_t* flip) try {
    using namespace hello;
    if (n_records < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (n_records > 0 && (!link || !chromosome || !set || !flip)) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (window < 1 || window > HELLO_PHASE_MAX_WINDOW) return set_last_error(HELLO_ERR_ARG, "window %d: 1 to %d", window, HELLO_PHASE_MAX_WINDOW);
    if (min_margin < 1) return set_last_error(HELLO_ERR_ARG, "min_margin %d: at least 1", min_margin);
    if (n_records > INT32_MAX) return set_last_error(HELLO_ERR_ARG, "%lld records", (long long)n_records);
    for (int64_t t = 0; t < n_records; ++t) {
        int32_t seen[HELLO_PHASE_MAX_WINDOW];                               // the sets met, in the order of k
        int64_t same[HELLO_PHASE_MAX_WINDOW], opp[HELLO_PHASE_MAX_WINDOW];
        int n_seen = 0;
        for (int k = 1; k <= window && t - k >= 0; ++k) {
            const int64_t s = t - k;
            if (chromosome[s] != chromosome[t]) continue;
            int64_t cis = link[(t * window + (k - 1)) * 2], trans = link[(t * window + (k - 1)) * 2 + 1];
            if (flip[s]) std::swap(cis, trans);
            int g = 0;
            while (g < n_seen && seen[g] != set[s]) ++g;
            if (g == n_seen) {
                seen[g] = set[s];
                same[g] = opp[g] = 0;
                ++n_seen;
            }
            same[g] += cis;
            opp[g] += trans;
        }
        int best = -1;
        int64_t margin = -1;
        for (int g = 0; g < n_seen; ++g) {
            const int64_t m = same[g] > opp[g] ? same[g] - opp[g] : opp[g] - same[g];
            if (m > margin) { margin = m; best = g; }                      // a tie stays with the set of the smaller k
        }
        if (best >= 0 && margin >= min_margin) {
            set[t] = seen[best];
            flip[t] = opp[best] > same[best] ? 1 : 0;
        } else {
            set[t] = (int32_t)t;
            flip[t] = 0;
        }
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_phase_chain")

int hello_phase_tag(hello_phase* h, const int32_t* set, const uint8_t* flip) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!h || (h->n_records > 0 && (!set || !flip))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    const int64_t n = h->n_records;
    const std::vector<int64_t> set_pos = set_positions(h, set, flip);
    h->hp.assign((size_t)h->n_reads, 0);
    h->ps.assign((size_t)h->n_reads, 0);
    h->stats[6] = 0.0;
    bool any = false;
    for (const PhBatch& b : h->batches) any = any || b.n_slots > 0;
    if (any) {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        PhTagArgs a{};
        a.set = m.put(set, (size_t)n);
        a.flip = m.put(flip, (size_t)n);
        a.set_pos = m.put(set_pos.data(), set_pos.size());
        KernelTimer timer;
        for (const PhBatch& b : h->batches) {
            if (b.n_slots == 0) continue;
            a.slots = b.slots;
            a.slot_off = b.slot_off;
            a.first = b.first;
            a.n_counted = b.n_counted;
            a.hp = m.zeros<uint8_t>((size_t)b.n_counted);
            a.ps = m.zeros<int64_t>((size_t)b.n_counted);
            timer.start();
            hipLaunchKernelGGL(phase_tag_kernel, dim3(blocks_for(b.n_counted, kPhThreads)), dim3(kPhThreads), 0, 0, a);
            h->stats[6] += timer.stop();
            std::vector<uint8_t> hp((size_t)b.n_counted);
            std::vector<int64_t> ps((size_t)b.n_counted);
            HS_HIP(hipMemcpy(hp.data(), a.hp, hp.size(), hipMemcpyDeviceToHost));
            HS_HIP(hipMemcpy(ps.data(), a.ps, ps.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < b.n_counted; ++k) {
                h->hp[(size_t)(b.read_base + b.reads[k])] = hp[k];
                h->ps[(size_t)(b.read_base + b.reads[k])] = ps[k];
            }
        }
    }
    h->stats[8] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    return HELLO_OK;
} HS_ENTRY_END("hello_phase_tag")

int hello_phase_fragments(hello_phase* h, const uint64_t* name_hash, const uint16_t* flags, const uint8_t* source,
                          int64_t n_reads) try {
    using namespace hello;
    if (!h) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads != h->n_reads)
        return set_last_error(HELLO_ERR_ARG, "n_reads %lld: the handle holds %lld reads", (long long)n_reads, (long long)h->n_reads);
    if (n_reads > 0 && (!name_hash || !flags || !source)) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (!h->hp.empty() || !h->ps.empty()) return set_last_error(HELLO_ERR_ARG, "mates cannot be joined after a tag call");
    if (h->fragments) return set_last_error(HELLO_ERR_ARG, "hello_phase_fragments is called once, after the last hello_phase_observe");
    for (int64_t r = 0; r < n_reads; ++r)
        if (source[r] > 1) return set_last_error(HELLO_ERR_ARG, "source[%lld] = %d: 0 or 1", (long long)r, (int)source[r]);

    // ---- the counted reads of all batches as one set, c = 0..n-1 in the order given, and their slots in the joined array
    std::vector<int64_t> reads;
    for (const PhBatch& b : h->batches)
        for (int64_t r : b.reads) reads.push_back(b.read_base + r);
    const int64_t n = (int64_t)reads.size(), n_slots = (int64_t)h->slots.size();
    if (n > kPairMaxReads) return set_last_error(HELLO_ERR_ARG, "%lld counted reads in one chromosome", (long long)n);
    std::vector<uint64_t> name((size_t)n);
    std::vector<uint16_t> fl((size_t)n);
    std::vector<uint8_t> src((size_t)n);
    std::vector<int64_t> first((size_t)n), slot_off((size_t)n + 1, n_slots);
    for (int64_t c = 0; c < n; ++c) {
        const size_t r = (size_t)reads[c];
        name[c] = name_hash[r];
        fl[c] = flags[r];
        src[c] = source[r];
        first[c] = h->first[r];
        slot_off[c] = h->slot_offsets[r];                                  // an uncounted read has no slot: c's slots end where
    }                                                                       // those of c + 1 begin
    std::vector<int32_t> mate((size_t)n, -1), link(h->links.size(), 0);
    int32_t totals[2] = {0, 0};
    float pair_ms = 0.0f, link_ms = 0.0f;
    if (n > 0) {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        for (void* p : {(void*)h->d_frag_slot_off, (void*)h->d_frag_first, (void*)h->d_frag_mate, (void*)h->d_frag_slots})
            (void)hipFree(p);                                              // what a refused earlier call left
        h->d_frag_slot_off = h->d_frag_first = nullptr;
        h->d_frag_mate = nullptr;
        h->d_frag_slots = nullptr;
        const auto take = [&m](auto* p) { return m.release(p); };         // to the handle at once, as in hello_phase_observe
        h->d_frag_slot_off = take(m.put(slot_off.data(), slot_off.size()));
        h->d_frag_first = take(m.put(first.data(), first.size()));
        h->d_frag_mate = take(m.room<int32_t>((size_t)n));
        h->d_frag_slots = take(m.room<int8_t>((size_t)n_slots));
        int64_t at = 0;
        for (const PhBatch& b : h->batches) {                              // the slots stay on the device: joined there
            if (b.n_slots > 0) HS_HIP(hipMemcpy(h->d_frag_slots + at, b.slots, (size_t)b.n_slots, hipMemcpyDeviceToDevice));
            at += b.n_slots;
        }
        if (at != n_slots) raise(HELLO_ERR_SHAPE, "the batches hold %lld slots, the handle %lld", (long long)at, (long long)n_slots);
        pair_ms = pair_join(m, m.put(name.data(), name.size()), m.put(fl.data(), fl.size()), m.put(src.data(), src.size()), n,
                            h->d_frag_mate, totals);
        HS_HIP(hipMemcpy(mate.data(), h->d_frag_mate, mate.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        KernelTimer timer;
        if (n_slots > 0) {
            PhFragArgs a{};
            a.slots = h->d_frag_slots;
            a.slot_off = h->d_frag_slot_off;
            a.first = h->d_frag_first;
            a.mate = h->d_frag_mate;
            a.link = m.zeros<int32_t>(link.size());
            a.n_slots = n_slots;
            a.n_counted = n;
            a.window = h->window;
            timer.start();
            hipLaunchKernelGGL(phase_fragment_link_kernel, dim3(blocks_for(n_slots, kPhThreads)), dim3(kPhThreads), 0, 0, a);
            link_ms = timer.stop();
            HS_HIP(hipMemcpy(link.data(), a.link, link.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    }
    h->mate.assign((size_t)n_reads, -1);
    for (int64_t c = 0; c < n; ++c)
        if (mate[c] >= 0) h->mate[(size_t)reads[c]] = reads[mate[c]];
    h->fragment_links.swap(link);
    h->counted_reads.swap(reads);
    h->n_counted = n;
    h->n_slots = n_slots;
    h->fragment_stats[0] = (double)totals[0];
    h->fragment_stats[1] = (double)totals[1];
    h->fragment_stats[2] = pair_ms;
    h->fragment_stats[3] = link_ms;
    h->fragments = true;
    return HELLO_OK;
} HS_ENTRY_END("hello_phase_fragments")

int hello_phase_tag_fragments(hello_phase* h, const int32_t* set, const uint8_t* flip) try {
    using namespace hello;
    if (!h || (h->n_records > 0 && (!set || !flip))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (!h->fragments) return set_last_error(HELLO_ERR_ARG, "hello_phase_tag_fragments needs hello_phase_fragments before it");
    const std::vector<int64_t> set_pos = set_positions(h, set, flip);
    h->hp.assign((size_t)h->n_reads, 0);
    h->ps.assign((size_t)h->n_reads, 0);
    h->fragment_stats[4] = 0.0;
    if (h->n_slots > 0) {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        const size_t n = (size_t)h->n_counted;
        PhFragArgs a{};
        a.slots = h->d_frag_slots;
        a.slot_off = h->d_frag_slot_off;
        a.first = h->d_frag_first;
        a.mate = h->d_frag_mate;
        a.n_slots = h->n_slots;
        a.n_counted = h->n_counted;
        a.window = h->window;
        a.set = m.put(set, (size_t)h->n_records);
        a.flip = m.put(flip, (size_t)h->n_records);
        a.set_pos = m.put(set_pos.data(), set_pos.size());
        a.hp = m.room<uint8_t>(n);
        a.ps = m.room<int64_t>(n);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(phase_fragment_tag_kernel, dim3(blocks_for(h->n_counted, kPhThreads)), dim3(kPhThreads), 0, 0, a);
        h->fragment_stats[4] = timer.stop();
        std::vector<uint8_t> hp(n);
        std::vector<int64_t> ps(n);
        HS_HIP(hipMemcpy(hp.data(), a.hp, n, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(ps.data(), a.ps, n * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < n; ++c) {
            h->hp[(size_t)h->counted_reads[c]] = hp[c];
            h->ps[(size_t)h->counted_reads[c]] = ps[c];
        }
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_phase_tag_fragments")

int hello_phase_array(const hello_phase* h, int32_t which, const void** data, int64_t* count) {
    if (!h || !data || !count) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    switch (which) {
        case HELLO_PHASE_SLOTS: *data = h->slots.data(); *count = (int64_t)h->slots.size(); break;
        case HELLO_PHASE_SLOT_OFFSETS: *data = h->slot_offsets.data(); *count = (int64_t)h->slot_offsets.size(); break;
        case HELLO_PHASE_FIRST: *data = h->first.data(); *count = (int64_t)h->first.size(); break;
        case HELLO_PHASE_LINKS: *data = h->links.data(); *count = (int64_t)h->links.size(); break;
        case HELLO_PHASE_HP: *data = h->hp.data(); *count = (int64_t)h->hp.size(); break;
        case HELLO_PHASE_PS: *data = h->ps.data(); *count = (int64_t)h->ps.size(); break;
        case HELLO_PHASE_MATE: *data = h->mate.data(); *count = (int64_t)h->mate.size(); break;
        case HELLO_PHASE_FRAGMENT_LINKS: *data = h->fragment_links.data(); *count = (int64_t)h->fragment_links.size(); break;
        default: return hello::set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
}

int hello_phase_stats(const hello_phase* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_PHASE_STATS, stats);
    return HELLO_OK;
}

int hello_phase_fragment_stats(const hello_phase* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->fragment_stats, h->fragment_stats + HELLO_PHASE_FRAGMENT_STATS, stats);
    return HELLO_OK;
}

void hello_phase_free(hello_phase* h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;
}

}  // extern "C"
