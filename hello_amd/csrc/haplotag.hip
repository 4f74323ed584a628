// Haplotags from a phased VCF (include/hello_mi355x.h: hello_haplotag_*): aligned reads + the phased records of one chromosome
// (span, haplotype-1 allele, haplotype-2 allele, phase set) -> hp (1, 2 or 0) and ps of every read.  Not in the reference;
// DESIGN.md section 7h states the rule and hello_amd/haplotag.py restates it in Python, integer for integer.
//
// The handle keeps the record table on the device: it is uploaded once per chromosome and read by every call, one call per read
// set (the candidate stages call once per shard file).  Host, per call: the read filter and the validation of every counted read
// (cigar.h: the kernel reads within its bases), which also gives the read's reference end; nothing else -- no candidate range, no
// scan, no slot.  Device, ONE kernel: a wave per read.
//   - the read's candidate records [t0, t1) come from two lower-bound searches in the device-resident record starts, done by the
//     wave together, 64 probes and one ballot per step (ht_lower_bound); the second starts at t0 with the 64 records behind it.
//     Most reads of a short-read set have no candidate, so the searches ARE their cost: a search by halves, every lane alike,
//     took 20 dependent loads per read at 1 000 records and made the launch twice as slow as the two it replaces (section 7h);
//   - the lanes hold the candidates, 64 per round, in record order, and walk the CIGAR (phase_walk.h, the walk of phase.hip);
//   - after each round the wave reduces: a 64-bit ballot of the lanes with an observation; without a set so far, the lowest such
//     lane's PS becomes the set (one shuffle); two ballots of "PS == set and observation 0 / 1", whose popcounts add to n1 / n2.
//     set, n1 and n2 are wave-uniform and carried across the rounds, so sets may interleave along the chromosome;
//   - lane 0 writes hp[r] and ps[r].  Every read has a wave, also an uncounted one and one without a candidate: their wave writes
//     the zeros, so each output has exactly one writer and nothing is pre-filled.
// Every lane reaches every vote, ballot and shuffle: the only exits before them depend on the read alone.  Integers only, no
// atomics, no slot array: two runs give the same bytes.
#include <chrono>
#include <climits>
#include <memory>

#include "phase_walk.h"
#include "stage_host.h"

namespace hello {
namespace {

constexpr int kHtThreads = 256;                                          // as phase.hip: four waves, four reads per workgroup
constexpr int kHtWaves = kHtThreads / 64;

struct HtArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;      // [reads]: the reference end from the CIGAR of a counted read, -1 for an uncounted one
    const int64_t* rec_start;    // [records], sorted
    const int64_t* rec_end;
    const uint8_t* alleles;      // haplotype-1 then haplotype-2 allele of every record, upper case
    const int64_t* allele_off;   // [2 records + 1]
    const int64_t* rec_ps;       // [records], positive
    uint8_t* hp;                 // [reads]
    int64_t* ps;
    int64_t n_reads, n_records;
    int q_threshold;
};

// The first index of the sorted v[0, n) whose element is not below x, found by the wave together: each step the 64 lanes probe 64
// evenly spaced elements of [lo, hi) and one ballot narrows the range to the gap behind the last probe below x -- two dependent
// loads for 4 096 records where a search by halves takes twelve.  v, n and x are wave-uniform and EVERY lane calls it.
__device__ inline int64_t ht_lower_bound(const int64_t* v, int64_t n, int64_t x, int lane) {
    int64_t lo = 0, hi = n;                                              // v[i] < x below lo, v[i] >= x from hi on
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) / 64;                        // the probes lo, lo + step, ... reach hi
        const int64_t i = lo + lane * step;
        const int k = __popcll(__ballot(i < hi && v[i] < x));            // sorted: the probes below x are the first k
        if (k == 0) {
            hi = lo;
        } else {
            const int64_t next = lo + k * step;                          // the first probe not below x, or beyond the range
            lo = lo + (k - 1) * step + 1;
            hi = next < hi ? next : hi;
        }
    }
    return lo;
}

__global__ __launch_bounds__(kHtThreads) void haplotag_kernel(HtArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kHtWaves + (threadIdx.x >> 6);
    if (r >= a.n_reads) return;                                          // the whole wave
    const int64_t re = a.ref_end[r];
    int64_t set = 0;                                                     // wave-uniform from here on, with n1 and n2
    int n1 = 0, n2 = 0;
    if (re >= 0) {                                                       // a counted read: the whole wave, or none of it
        const int64_t rs = a.ref_start[r], c0 = a.cigar_off[r];
        const int64_t t0 = ht_lower_bound(a.rec_start, a.n_records, rs, lane);
        // the end of the range lies at or behind t0 (rs <= re), for most reads within the next 64 records: one probe of those first
        int64_t n_cand = __popcll(__ballot(t0 + lane < a.n_records && a.rec_start[t0 + lane] < re));
        if (n_cand == 64) n_cand += ht_lower_bound(a.rec_start + t0 + 64, a.n_records - t0 - 64, re, lane);
        const PhWalkRead rd{a.bases + a.read_off[r], a.quals + a.read_off[r], a.cigars + c0, a.cigar_off[r + 1] - c0, rs, re};
        const PhWalkTable tb{a.rec_start, a.rec_end, a.alleles, a.allele_off};
        for (int64_t round = 0; round < n_cand; round += 64) {
            const int64_t j = round + lane;
            const bool mine = j < n_cand;
            const int o = phase_walk_observe(rd, tb, t0 + j, mine, a.q_threshold);
            const int64_t my_ps = mine ? a.rec_ps[t0 + j] : 0;
            const unsigned long long seen = __ballot(o >= 0);
            if (set == 0 && seen != 0) set = __shfl(my_ps, __ffsll(seen) - 1);           // the first observation, in record order
            const bool in_set = o >= 0 && my_ps == set;
            n1 += __popcll(__ballot(in_set && o == 0));
            n2 += __popcll(__ballot(in_set && o == 1));
        }
    }
    if (lane == 0) {
        a.hp[r] = n1 > n2 ? 1 : n2 > n1 ? 2 : 0;
        a.ps[r] = set;
    }
}

}  // namespace
}  // namespace hello

struct hello_haplotag {
    int device = 0;
    int64_t n_records = 0;
    int64_t* d_rec_start = nullptr;
    int64_t* d_rec_end = nullptr;
    uint8_t* d_alleles = nullptr;
    int64_t* d_allele_off = nullptr;
    int64_t* d_ps = nullptr;
    double stats[HELLO_HAPLOTAG_STATS] = {0};
    ~hello_haplotag() {                                                     // without a record nothing was opened or allocated
        for (void* p : {(void*)d_rec_start, (void*)d_rec_end, (void*)d_alleles, (void*)d_allele_off, (void*)d_ps})
            if (p) (void)hipFree(p);
    }
};

extern "C" {

int hello_haplotag_create(const int64_t* record_starts, const int64_t* record_ends, const uint8_t* alleles,
                          const int64_t* allele_offsets, const int64_t* ps, int64_t n_records, int32_t device,
                          hello_haplotag** handle) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!handle || !allele_offsets || (n_records > 0 && (!record_starts || !record_ends || !alleles || !ps)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_records < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (n_records > INT32_MAX) return set_last_error(HELLO_ERR_ARG, "%lld records in one chromosome", (long long)n_records);
    if (allele_offsets[0] != 0) return set_last_error(HELLO_ERR_ARG, "allele_offsets[0] is not 0");
    for (int64_t t = 0; t < n_records; ++t) {
        if (record_starts[t] < 0 || record_ends[t] <= record_starts[t])
            return set_last_error(HELLO_ERR_ARG, "record %lld: span [%lld, %lld)", (long long)t, (long long)record_starts[t],
                                  (long long)record_ends[t]);
        if (t > 0 && record_starts[t] < record_starts[t - 1])
            return set_last_error(HELLO_ERR_ARG, "record %lld: records are not sorted by position", (long long)t);
        if (allele_offsets[2 * t + 1] < allele_offsets[2 * t] || allele_offsets[2 * t + 2] < allele_offsets[2 * t + 1])
            return set_last_error(HELLO_ERR_SHAPE, "record %lld: allele offsets decrease", (long long)t);
        if (ps[t] <= 0) return set_last_error(HELLO_ERR_ARG, "record %lld: phase set %lld is not positive", (long long)t, (long long)ps[t]);
    }
    std::unique_ptr<hello_haplotag> h(new hello_haplotag());
    h->n_records = n_records;
    h->device = device;
    h->stats[0] = (double)n_records;
    if (n_records > 0) {                                                    // without a record no call launches: no device is opened
        open_device(device);
        DevMem m;                                                           // each upload leaves to the handle at once
        h->d_rec_start = m.release(m.put(record_starts, (size_t)n_records));
        h->d_rec_end = m.release(m.put(record_ends, (size_t)n_records));
        h->d_alleles = m.release(m.put(alleles, (size_t)allele_offsets[2 * n_records]));
        h->d_allele_off = m.release(m.put(allele_offsets, (size_t)(2 * n_records + 1)));
        h->d_ps = m.release(m.put(ps, (size_t)n_records));
    }
    h->stats[8] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    *handle = h.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_haplotag_create")

int hello_haplotag_reads(hello_haplotag* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets,
                         const uint32_t* cigars, const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends,
                         const uint8_t* mapq, const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                         int32_t q_threshold, int32_t mapq_threshold, uint8_t* hp, int64_t* ps) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    (void)source;                                                           // a read is tagged alike whichever BAM it came from
    if (!h || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends || !mapq ||
        !flags || !name_hash || !hp || !ps)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if ((n_reads + hello::kHtWaves - 1) / hello::kHtWaves > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "%lld reads in one launch", (long long)n_reads);

    // ---- the counted reads, validated (the kernel reads within their bases), and their reference ends
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    std::vector<int64_t> ends((size_t)n_reads, -1);
    int64_t n_counted = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        int64_t qlen, rlen;
        if (!counted_walk(in, r, mapq_threshold, qlen, rlen)) continue;
        ends[(size_t)r] = ref_starts[r] + rlen;
        ++n_counted;
    }
    const auto t1 = clock::now();

    float kernel_ms = 0.0f;
    int64_t tagged[2] = {0, 0};
    if (n_counted == 0 || h->n_records == 0) {                             // nothing to launch: nobody has a candidate
        std::fill(hp, hp + n_reads, (uint8_t)0);
        std::fill(ps, ps + n_reads, (int64_t)0);
    } else {
        HS_HIP(hipSetDevice(h->device));
        DevMem m;
        HtArgs a{};
        const DeviceReads d = upload_reads(m, in);
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.ref_end = m.put(ends.data(), ends.size());
        a.rec_start = h->d_rec_start;
        a.rec_end = h->d_rec_end;
        a.alleles = h->d_alleles;
        a.allele_off = h->d_allele_off;
        a.rec_ps = h->d_ps;
        a.hp = m.room<uint8_t>((size_t)n_reads);                            // every read's wave writes both
        a.ps = m.room<int64_t>((size_t)n_reads);
        a.n_reads = n_reads;
        a.n_records = h->n_records;
        a.q_threshold = q_threshold;
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(haplotag_kernel, dim3((unsigned)((n_reads + kHtWaves - 1) / kHtWaves)), dim3(kHtThreads), 0, 0, a);
        kernel_ms = timer.stop();
        HS_HIP(hipMemcpy(hp, a.hp, (size_t)n_reads, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(ps, a.ps, (size_t)n_reads * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < n_reads; ++r)
            if (hp[r] == 1 || hp[r] == 2) ++tagged[hp[r] - 1];
    }
    h->stats[1] += 1.0;
    h->stats[2] += (double)n_reads;
    h->stats[3] += (double)n_counted;
    h->stats[4] += (double)tagged[0];
    h->stats[5] += (double)tagged[1];
    h->stats[6] += kernel_ms;
    h->stats[7] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->stats[8] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    return HELLO_OK;
} HS_ENTRY_END("hello_haplotag_reads")

int hello_haplotag_stats(const hello_haplotag* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_HAPLOTAG_STATS, stats);
    return HELLO_OK;
}

void hello_haplotag_free(hello_haplotag* h) {
    if (h && h->n_records > 0) (void)hipSetDevice(h->device);
    delete h;
}

}  // extern "C"
