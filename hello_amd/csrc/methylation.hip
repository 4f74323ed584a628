// CpG methylation per haplotype from the MM / ML calls of the reads (include/hello_mi355x.h: hello_meth_*): the chromosome's text
// and, span after span, its reads with their parsed modifications (mods.h) -> integer sums per CpG site.  Not in the reference;
// DESIGN.md section 7m states the rules and hello_amd/methylation.py restates them in Python, integer for integer.
//
// Host: the classes of the reads and the validation of every counted read (cigar.h: meth_walk) and of the modification arrays
// (mods.h: mods_walk) -- the kernels index with both -- and the scratch slices of the reads whose targets do not fit in LDS.
// Device, once per handle, three kernels over the reference:
//   flag: a wave per 64 positions; the ballot of "C here, G next" is the word of the site bit vector (site_bits.h).
//   scan: site_bits.h's, over the words' popcounts -> the sites before every word, which give a site its rank.
//   compact: a wave per word writes the positions of its set bits to SITES at their ranks.
// and per hello_meth_add one kernel, a workgroup per kMethChunkReads candidate reads, a wave per read:
//   step 1: the candidate bytes of the read ('C', or 'G' for a reverse read) are summed with ballots; the deltas are prefix-summed
//     64 at a time with a carry into the targets t_k = k + delta_0 + .. + delta_k (LDS, or the read's scratch slice); the read is
//     refused into its status byte when t_last is no candidate.
//   step 2: the CIGAR operation by operation (wave-uniform loop) with the lanes on an operation's bases (read_walk.h: the decoder).
//     Over every query-consuming operation the wave keeps the running count of candidates; a candidate lane inside M / = / X
//     looks up the site bit at its position, binary-searches its ordinal in the targets and adds to the site's nine counters.
// Every output is an integer sum, so no result depends on the order of the atomic adds: two runs give the same bytes.
#include <memory>

#include "mods.h"
#include "read_walk.h"
#include "site_bits.h"

namespace hello {
namespace {

constexpr int kMethThreads = 256;
constexpr int kMethWaves = kMethThreads / 64;
constexpr int kMethShare = 1024;             // targets of a wave's read in LDS; a read that lists more has a scratch slice
constexpr int kMethChunkReads = 4;           // reads per workgroup: a wave each, so that 2 000 long reads fill the chip
constexpr int kMethCounters = 9;             // [class][counter]

struct MethSitesArgs {
    const uint8_t* ref;
    int64_t length, n_words;
    unsigned long long* bits;    // [n_words]
    int* before;                 // [n_words + 1]
    int64_t* sites;              // [n_sites]
};

__global__ __launch_bounds__(kMethThreads) void meth_flag_kernel(MethSitesArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kMethWaves + wave;
    if (w >= a.n_words) return;                                           // the whole wave
    const int64_t p = w * 64 + lane;
    const bool site = p + 1 < a.length && (a.ref[p] & 0xDF) == 'C' && (a.ref[p + 1] & 0xDF) == 'G';
    const unsigned long long b = __ballot(site);
    if (lane == 0) a.bits[w] = b;
}

__global__ __launch_bounds__(kMethThreads) void meth_compact_kernel(MethSitesArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kMethWaves + wave;
    if (w >= a.n_words) return;
    const unsigned long long b = a.bits[w];
    if ((b >> lane) & 1ull) a.sites[a.before[w] + __popcll(b & ((1ull << lane) - 1ull))] = w * 64 + lane;
}

struct MethReadsArgs {
    const uint8_t* bases;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const uint16_t* flags;
    const uint8_t* hp;
    const int32_t* deltas;
    const uint8_t* probs;
    const int64_t* mod_off;
    const uint8_t* mode;
    const int64_t* list;         // [n_list]: the belonging counted reads without a hard clip whose state is 1, in input order
    const int64_t* scratch_off;  // [n_list]: where the read's targets go in `scratch`, or -1 for the wave's share of LDS
    int32_t* scratch;
    uint8_t* refused;            // [n_list]: 1 when the last listed base is no candidate of the read
    int64_t n_list;
    SiteBits sb;                 // the CpG sites
    unsigned* counts;            // [n_sites][3][3]
    unsigned long long* observations;
};

// Every lane adds straight to the global table: section 7m has the measurement against a workgroup that combines first.
__global__ __launch_bounds__(kMethThreads) void meth_reads_kernel(MethReadsArgs a) {
    __shared__ int targets[kMethWaves * kMethShare];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t k_lo = (int64_t)blockIdx.x * kMethChunkReads;
    const int64_t k_hi = k_lo + kMethChunkReads < a.n_list ? k_lo + kMethChunkReads : a.n_list;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t k = k_lo + wave; k < k_hi; k += kMethWaves) {
        const int64_t r = a.list[k];
        const int64_t q0 = a.read_off[r];
        const int len = (int)(a.read_off[r + 1] - q0);
        const bool reverse = (a.flags[r] & 0x10) != 0;
        const uint8_t candidate = reverse ? 'G' : 'C';
        const uint8_t* bases = a.bases + q0;

        // ---- step 1: the candidates of the read, and the ordinals of its listed bases
        int total = 0;
        for (int j0 = 0; j0 < len; j0 += 64) {
            const int j = j0 + lane;
            total += __popcll(__ballot(j < len && bases[j] == candidate));
        }
        const int64_t m0 = a.mod_off[r];
        const int n_targets = (int)(a.mod_off[r + 1] - m0);
        int* t = a.scratch_off[k] >= 0 ? a.scratch + a.scratch_off[k] : targets + wave * kMethShare;
        long long carry = 0;                                              // listed bases and skipped ones so far
        for (int k0 = 0; k0 < n_targets; k0 += 64) {
            const int kk = k0 + lane;
            long long s = kk < n_targets ? (long long)a.deltas[m0 + kk] + 1 : 0;
            for (int d = 1; d < 64; d <<= 1) {
                const long long up = __shfl_up(s, d, 64);
                if (lane >= d) s += up;
            }
            if (kk < n_targets) {
                const long long ordinal = carry + s - 1;                  // t_k = k + delta_0 + .. + delta_k
                t[kk] = ordinal > INT32_MAX ? INT32_MAX : (int)ordinal;   // past every read's end: the read is refused below
            }
            carry += __shfl(s, 63, 64);
        }
        const bool refused = n_targets > 0 && carry - 1 >= total;
        if (lane == 0) a.refused[k] = refused ? 1 : 0;
        if (refused) continue;                                            // the whole wave
        __threadfence_block();                                            // the lanes read each other's targets

        // ---- step 2: the walk
        const int unknown = a.mode[r];
        const int hp = a.hp[r];
        const int cls = hp == 1 || hp == 2 ? hp : 0;
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = a.ref_start[r];
        int rd = 0, running = 0, n_obs = 0;
        for (int64_t ci = 0; ci < n_ops; ++ci) {
            const CigarOp o = decode_op(a.cigars[c0 + ci]);
            const int n = o.n;
            if (o.on_read()) {
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int j = j0 + lane;
                    const bool is_candidate = j < n && bases[rd + j] == candidate;       // rd + n <= len: meth_walk
                    const unsigned long long all = __ballot(is_candidate);
                    bool observed = false;
                    if (o.m && is_candidate) {
                        const int from_left = running + __popcll(all & below);
                        const int ordinal = reverse ? total - 1 - from_left : from_left;
                        const int64_t pos = rf + j, p = reverse ? pos - 1 : pos;
                        if (pos < a.sb.length && p >= 0) {
                            const unsigned long long w = a.sb.word(p);
                            if (SiteBits::has(w, p)) {
                                int x = 0, y = n_targets;                     // the first target at or above the ordinal
                                while (x < y) {
                                    const int mid = (x + y) >> 1;
                                    if (t[mid] < ordinal) x = mid + 1; else y = mid;
                                }
                                const bool is_listed = x < n_targets && t[x] == ordinal;
                                if (is_listed || !unknown) {
                                    observed = true;
                                    const int v = is_listed ? a.probs[m0 + x] : 0;
                                    const int rank = a.sb.rank(w, p);
                                    const int counter = v >= 128 ? 0 : 1;
                                    for (int which = 0; which <= cls; which += cls ? cls : 1) {
                                        unsigned* e = a.counts + (int64_t)rank * kMethCounters + which * 3;
                                        atomicAdd(e + counter, 1u);
                                        if (v) atomicAdd(e + 2, (unsigned)v);
                                    }
                                }
                            }
                        }
                    }
                    n_obs += __popcll(__ballot(observed));
                    running += __popcll(all);                             // over every operation that consumes the read
                }
                rd += n;
                if (o.m) rf += n;
            } else if (o.op == BAM_CDEL || o.op == BAM_CREF_SKIP) {
                rf += n;
            }
        }
        if (lane == 0 && n_obs) atomicAdd(a.observations, (unsigned long long)n_obs);
    }
}

}  // namespace
}  // namespace hello

struct hello_meth : hello::SpanHandle<HELLO_METH_STATS> {
    int32_t mapq_threshold = 0;
    hello::DevMem mem;                           // bits and before live as long as the handle
    hello::SiteBits sb{};
    hello::CountTable counts;                    // [n_sites][3][3]
    std::vector<int64_t> sites;
    bool built = false;
    std::vector<uint8_t> reference;              // until the device side is built
};

extern "C" {

// The device side of a handle, built when the first hello_meth_add has passed its checks (or an array is asked for): the
// reference goes up, the three site kernels run, SITES comes back and the reference is dropped on both sides.
static void meth_build_sites(hello_meth* h) {
    using namespace hello;
    if (h->built) return;
    open_device(h->device);
    MethSitesArgs a{};
    DevMem keep, m;                              // m: what only the site kernels need
    a.ref = m.put(h->reference.data(), h->reference.size());
    a.length = h->length;
    a.n_words = (h->length + 63) / 64;
    a.bits = keep.room<unsigned long long>((size_t)a.n_words);
    a.before = keep.room<int>((size_t)a.n_words + 1);
    const unsigned blocks = (unsigned)((a.n_words + kMethWaves - 1) / kMethWaves);
    KernelTimer timer;
    float ms = 0.0f;
    timer.start();
    if (blocks) hipLaunchKernelGGL(meth_flag_kernel, dim3(blocks), dim3(kMethThreads), 0, 0, a);
    const int n_sites = build_scan(timer, a.bits, a.before, a.n_words, ms);
    a.sites = m.room<int64_t>((size_t)n_sites);
    timer.start();
    if (blocks) hipLaunchKernelGGL(meth_compact_kernel, dim3(blocks), dim3(kMethThreads), 0, 0, a);
    ms += timer.stop();
    std::vector<int64_t> sites((size_t)n_sites);
    if (n_sites) HS_HIP(hipMemcpy(sites.data(), a.sites, (size_t)n_sites * sizeof(int64_t), hipMemcpyDeviceToHost));
    CountTable counts;
    counts.build((size_t)n_sites * kMethCounters);
    // ---- nothing can fail from here on
    h->mem.ptrs.swap(keep.ptrs);
    h->sb = SiteBits{a.bits, a.before, a.length, a.n_words};
    h->counts.swap(counts);
    h->sites.swap(sites);
    std::vector<uint8_t>().swap(h->reference);
    h->stats[7] = (double)n_sites;
    h->stats[8] = ms;
    h->built = true;
}

int hello_meth_create(const uint8_t* reference, int64_t reference_length, int32_t mapq_threshold, int32_t device,
                      hello_meth** handle) try {
    using namespace hello;
    if (!reference || !handle) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *handle = nullptr;
    if (reference_length < 0 || reference_length > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "reference of %lld bases: 0 to %d", (long long)reference_length, INT32_MAX);
    std::unique_ptr<hello_meth> h(new hello_meth());
    h->device = device;
    h->mapq_threshold = mapq_threshold;
    h->length = reference_length;
    h->reference.assign(reference, reference + reference_length);
    *handle = h.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_meth_create")

int hello_meth_add(hello_meth* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                   const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                   const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads, const int32_t* deltas,
                   int64_t n_deltas, const uint8_t* probs, int64_t n_probs, const int64_t* mod_offsets, const uint8_t* mode,
                   const uint8_t* state, int64_t lo, int64_t hi) try {
    using namespace hello;
    (void)quals; (void)name_hash;
    if (!h || !read_offsets || !cigar_offsets || !mod_offsets || (n_reads > 0 && (!bases || !cigars || !ref_starts || !ref_ends ||
        !mapq || !flags || !hp || !mode || !state)) || (n_deltas > 0 && (!deltas || !probs)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    h->check_span(lo, hi);

    // ---- the reads and their modifications: validated, then the kernel's list and the scratch slices
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    const std::vector<uint8_t> kind = meth_walk(in, lo, h->mapq_threshold);
    const ModsView mods{deltas, probs, mod_offsets, mode, state, n_deltas, n_probs};
    mods_walk(mods, n_reads);
    std::vector<uint8_t> status((size_t)n_reads, 0);
    std::vector<int64_t> list, scratch_off;
    int64_t n_belonging = 0, n_none = 0, n_bad = 0, n_hard = 0, n_scratch = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        const uint8_t k = kind[(size_t)r];
        if (!(k & kMethBelongs)) continue;
        ++n_belonging;
        if (!(k & kMethCounted)) continue;
        if (k & kMethHardClipped) { status[(size_t)r] = 4; ++n_hard; continue; }
        if (state[r] == kModsNone) { status[(size_t)r] = 3; ++n_none; continue; }
        if (state[r] == kModsBad) { status[(size_t)r] = 2; ++n_bad; continue; }
        const int64_t n_t = mod_offsets[r + 1] - mod_offsets[r];
        if (n_t > INT32_MAX) raise(HELLO_ERR_ARG, "read %lld: %lld listed bases, at most %d", (long long)r, (long long)n_t, INT32_MAX);
        list.push_back(r);
        scratch_off.push_back(n_t > kMethShare ? n_scratch : -1);
        if (n_t > kMethShare) n_scratch += n_t;
    }
    const int64_t n_list = (int64_t)list.size();
    h->take_counting(n_list, kMethMaxReads, "sums");
    const int64_t n_blocks = (n_list + kMethChunkReads - 1) / kMethChunkReads;

    meth_build_sites(h);
    HS_HIP(hipSetDevice(h->device));
    std::vector<uint8_t> refused((size_t)n_list, 0);
    unsigned long long observations = 0;
    float reads_ms = 0.0f;
    if (n_list > 0) {
        DevMem m;
        const DeviceReads d = upload_reads(m, in);
        MethReadsArgs a{};
        a.bases = d.bases; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off; a.ref_start = d.ref_start;
        a.flags = m.put(flags, (size_t)n_reads);
        a.hp = m.put(hp, (size_t)n_reads);
        a.deltas = m.put(deltas, (size_t)n_deltas);
        a.probs = m.put(probs, (size_t)n_deltas);
        a.mod_off = m.put(mod_offsets, (size_t)n_reads + 1);
        a.mode = m.put(mode, (size_t)n_reads);
        a.list = m.put(list.data(), list.size());
        a.scratch_off = m.put(scratch_off.data(), scratch_off.size());
        a.scratch = m.room<int32_t>((size_t)n_scratch);
        a.refused = m.zeros<uint8_t>((size_t)n_list);
        a.n_list = n_list;
        a.sb = h->sb;
        a.counts = h->counts.device;
        a.observations = m.zeros<unsigned long long>(1);
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(meth_reads_kernel, dim3((unsigned)n_blocks), dim3(kMethThreads), 0, 0, a);
        reads_ms = timer.stop();
        h->counts.fetched = false;
        HS_HIP(hipMemcpy(refused.data(), a.refused, (size_t)n_list, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(&observations, a.observations, sizeof(observations), hipMemcpyDeviceToHost));
    }

    // ---- nothing can fail from here on
    int64_t n_counting = 0;
    for (int64_t k = 0; k < n_list; ++k) {
        status[(size_t)list[(size_t)k]] = refused[(size_t)k] ? 2 : 1;
        if (refused[(size_t)k]) ++n_bad; else ++n_counting;
    }
    h->status = std::move(status);
    h->counting_given += n_list;
    h->last_hi = hi;
    h->stats[0] += (double)n_reads;
    h->stats[1] += (double)n_belonging;
    h->stats[2] += (double)n_counting;
    h->stats[3] += (double)n_none;
    h->stats[4] += (double)n_bad;
    h->stats[5] += (double)n_hard;
    h->stats[6] += (double)observations;
    h->stats[9] += reads_ms;
    return HELLO_OK;
} HS_ENTRY_END("hello_meth_add")

int hello_meth_array(hello_meth* h, int32_t which, const void** data, int64_t* count) try {
    using namespace hello;
    if (!h || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (which == HELLO_METH_SITES || which == HELLO_METH_COUNTS) meth_build_sites(h);
    switch (which) {
        case HELLO_METH_SITES: *data = h->sites.data(); *count = (int64_t)h->sites.size(); break;
        case HELLO_METH_COUNTS: *data = h->counts.fetch(h->device).data(); *count = (int64_t)h->counts.host.size(); break;
        case HELLO_METH_STATUS: *data = h->status.data(); *count = (int64_t)h->status.size(); break;
        default: return set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_meth_array")

int hello_meth_stats(const hello_meth* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    return h->copy_stats(stats);
}

void hello_meth_free(hello_meth* h) { delete h; }

}  // extern "C"
