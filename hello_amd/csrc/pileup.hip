// Base counts per strand at a given list of sites (include/hello_mi355x.h: hello_pileup_*), and the entry points of the
// contamination and identity estimates on top of them (hello_contam_*; contam.h).  Not in the reference; DESIGN.md section 7n states
// the rules and hello_amd/contamination.py restates them in Python, integer for integer.
//
// Host: the classes of the reads and the validation of every counted read (cigar.h: pileup_walk) -- the kernels index with it.
// Device, once per handle, two kernels over the uploaded positions:
//   set:  a lane per site ORs its bit into the 64-position word of the site bit vector.
//   scan: site_bits.h's, over the words' popcounts -> the sites before every word.  The positions ascend, so the rank of the
//     site at p (SiteBits::rank) is its index in the list.
// and per hello_pileup_add one kernel, a workgroup per `share` counting reads (at most kPileShare; sized for kPileGroups workgroups):
//   phase 1, a lane per read: the words of the bit vector under [ref_start, ref_end) are ORed, two to four for a short read; the
//     reads that cover a site are compacted into LDS with ballots and popcounts.  A site list is sparse and most short reads cover
//     none, so most reads end here without their CIGAR being read.
//   phase 2, a wave per surviving read: the CIGAR operation by operation (wave-uniform loop) with the lanes on an operation's
//     bases (read_walk.h: the decoder).  A lane in M / = / X / D tests its position's bit and on a hit adds 1 to
//     COUNTS[rank][strand][bin] in global memory.
//   The plain form (HELLO_PILEUP_FORM 1) skips phase 1: every counting read is walked.  Section 7n has both measured.
// Every output is an integer sum, so no result depends on the order of the atomic adds: two runs give the same bytes.
#include <memory>

#include "contam.h"
#include "read_walk.h"
#include "site_bits.h"

namespace hello {
namespace {

constexpr int kPileThreads = 256;
constexpr int kPileWaves = kPileThreads / 64;
constexpr int kPileShare = 1024;             // the most counting reads of a workgroup: rounds of phase 1, then its four waves share phase 2
constexpr int kPileGroups = 4096;            // the share of a launch is sized for about so many workgroups: 2 000 long reads get a
                                             // wave each, 200 000 short ones 49 to a workgroup, a chromosome's 50 M the whole 1 024
constexpr int kPileBins = HELLO_PILEUP_BINS;
constexpr int kBinOther = 4, kBinDel = 5, kBinLowq = 6;

struct PileSitesArgs {
    const int64_t* pos;          // [n_sites]
    int64_t n_sites, n_words;
    unsigned long long* bits;    // [n_words], zeroed
    int* before;                 // [n_words + 1]
};

__global__ __launch_bounds__(kPileThreads) void pile_set_kernel(PileSitesArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kPileThreads + threadIdx.x;
    if (i >= a.n_sites) return;
    const int64_t p = a.pos[i];                                           // inside the chromosome: hello_pileup_create
    atomicOr(a.bits + (p >> 6), 1ull << (p & 63));
}

struct PileReadsArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;
    const uint16_t* flags;
    const int64_t* list;         // [n_list]: the belonging counted reads, in input order
    uint8_t* seen;               // [n_list], zeroed: 1 when the read made an observation
    int64_t n_list;
    SiteBits sb;                 // the sites given
    int q_threshold, share;      // share: the counting reads of a workgroup, 1 .. kPileShare
    unsigned* counts;            // [n_sites][2][7]
    unsigned long long* group_obs;   // [workgroups]: the observations of each
};

// Integer adds of 1 straight to the global table: a read meets few sites, so there is nothing for a workgroup to combine.
template <bool kTwoPhase>
__global__ __launch_bounds__(kPileThreads) void pile_reads_kernel(PileReadsArgs a) {
    __shared__ int survivors[kPileShare];
    __shared__ int wave_count[kPileWaves];
    __shared__ unsigned long long wave_total[kPileWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t k_lo = (int64_t)blockIdx.x * a.share;
    const int n_mine = (int)(k_lo + a.share < a.n_list ? a.share : a.n_list - k_lo);
    int n_walk = n_mine;
    if (kTwoPhase) {
        // ---- phase 1: a lane per read
        const unsigned long long below = (1ull << lane) - 1ull;
        n_walk = 0;
        for (int base = 0; base < n_mine; base += kPileThreads) {             // block-uniform
            const int i = base + tid;
            bool hit = false;
            if (i < n_mine) {
                const int64_t r = a.list[k_lo + i];
                const int64_t e = a.ref_end[r] < a.sb.length ? a.ref_end[r] : a.sb.length;
                hit = a.sb.any_in(a.ref_start[r], e);
            }
            const unsigned long long b = __ballot(hit);
            if (lane == 0) wave_count[wave] = __popcll(b);
            __syncthreads();
            int pre = 0, total = 0;
            for (int k = 0; k < kPileWaves; ++k) {
                if (k < wave) pre += wave_count[k];
                total += wave_count[k];
            }
            if (hit) survivors[n_walk + pre + __popcll(b & below)] = i;       // below n_mine <= kPileShare entries in all
            n_walk += total;
            __syncthreads();
        }
    }

    // ---- phase 2: a wave per read
    unsigned long long wave_obs = 0;
    for (int s = wave; s < n_walk; s += kPileWaves) {
        const int64_t k = k_lo + (kTwoPhase ? survivors[s] : s);
        const int64_t r = a.list[k];
        const int64_t q0 = a.read_off[r];
        const int strand = (a.flags[r] & 0x10) ? 1 : 0;
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = a.ref_start[r], rd = 0;
        int n_obs = 0;
        for (int64_t ci = 0; ci < n_ops; ++ci) {
            const CigarOp o = decode_op(a.cigars[c0 + ci]);
            const int n = o.n;
            if (o.m || o.op == BAM_CDEL) {
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int j = j0 + lane;
                    const int64_t p = rf + j;                                 // rf >= 0: pileup_walk
                    bool observed = false;
                    if (j < n && p < a.sb.length) {
                        const unsigned long long w = a.sb.word(p);
                        if (SiteBits::has(w, p)) {
                            int bin = kBinDel;
                            if (o.m) {                                        // rd + n <= the read's bases: pileup_walk
                                const int b = a.bases[q0 + rd + j] & 0xDF;
                                bin = a.quals[q0 + rd + j] < a.q_threshold ? kBinLowq
                                      : b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : kBinOther;
                            }
                            const int64_t rank = a.sb.rank(w, p);
                            atomicAdd(a.counts + (rank * 2 + strand) * kPileBins + bin, 1u);
                            observed = true;
                        }
                    }
                    n_obs += __popcll(__ballot(observed));
                }
                rf += n;
                if (o.m) rd += n;
            } else if (o.op == BAM_CINS || o.op == BAM_CSOFT_CLIP) {
                rd += n;
            } else if (o.op == BAM_CREF_SKIP) {
                rf += n;
            }
        }
        if (lane == 0 && n_obs) a.seen[k] = 1;
        wave_obs += (unsigned long long)n_obs;
    }
    // the workgroup's observations as one plain store, summed by the host: reads adding to one shared total serialise (section 7n)
    if (lane == 0) wave_total[wave] = wave_obs;
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0;
        for (int k = 0; k < kPileWaves; ++k) sum += wave_total[k];
        a.group_obs[blockIdx.x] = sum;
    }
}

}  // namespace
}  // namespace hello

struct hello_pileup : hello::SpanHandle<HELLO_PILEUP_STATS> {
    int form = 0, share = 0;                     // share 0: sized by the launch
    int32_t q_threshold = 0, mapq_threshold = 0;
    int64_t n_sites = 0;
    hello::DevMem mem;                           // bits and before live as long as the handle
    hello::SiteBits sb{};
    hello::CountTable counts;                    // [n_sites][2][7]
    std::vector<int64_t> pos;                    // until the device side is built
    bool built = false;
};

extern "C" {

// The device side of a handle, built when the first hello_pileup_add has passed its checks (or COUNTS is asked for).
static void pile_build_sites(hello_pileup* h) {
    using namespace hello;
    if (h->built) return;
    open_device(h->device);
    PileSitesArgs a{};
    DevMem keep, m;
    a.pos = m.put(h->pos.data(), h->pos.size());
    a.n_sites = h->n_sites;
    a.n_words = (h->length + 63) / 64;
    a.bits = keep.zeros<unsigned long long>((size_t)a.n_words);
    a.before = keep.room<int>((size_t)a.n_words + 1);
    CountTable counts;
    counts.build((size_t)h->n_sites * 2 * kPileBins);
    const unsigned blocks = (unsigned)((h->n_sites + kPileThreads - 1) / kPileThreads);
    KernelTimer timer;
    float ms = 0.0f;
    timer.start();
    if (blocks) hipLaunchKernelGGL(pile_set_kernel, dim3(blocks), dim3(kPileThreads), 0, 0, a);
    build_scan(timer, a.bits, a.before, a.n_words, ms);                // -> n_sites: the positions ascend strictly
    // ---- nothing can fail from here on
    h->mem.ptrs.swap(keep.ptrs);
    h->sb = SiteBits{a.bits, a.before, h->length, a.n_words};
    h->counts.swap(counts);
    std::vector<int64_t>().swap(h->pos);
    h->stats[6] = ms;
    h->built = true;
}

int hello_pileup_create(const int64_t* pos, int64_t n_sites, int64_t chromosome_length, int32_t q_threshold, int32_t mapq_threshold,
                        int32_t device, hello_pileup** handle) try {
    using namespace hello;
    if (!handle || (n_sites > 0 && !pos)) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *handle = nullptr;
    if (n_sites < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (chromosome_length < 0 || chromosome_length > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "chromosome of %lld bases: 0 to %d", (long long)chromosome_length, INT32_MAX);
    for (int64_t i = 0; i < n_sites; ++i) {
        if (pos[i] < 0 || pos[i] >= chromosome_length)
            return set_last_error(HELLO_ERR_ARG, "site %lld: position %lld of a chromosome of %lld bases", (long long)i, (long long)pos[i],
                                  (long long)chromosome_length);
        if (i > 0 && pos[i] <= pos[i - 1])
            return set_last_error(HELLO_ERR_ARG, "site %lld: position %lld is not above %lld before it", (long long)i, (long long)pos[i],
                                  (long long)pos[i - 1]);
    }
    std::unique_ptr<hello_pileup> h(new hello_pileup());
    h->device = device;
    h->q_threshold = q_threshold;
    h->mapq_threshold = mapq_threshold;
    h->length = chromosome_length;
    h->n_sites = n_sites;
    h->pos.assign(pos, pos + n_sites);
    h->stats[5] = (double)n_sites;
    *handle = h.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_pileup_create")

int hello_pileup_option(hello_pileup* h, int32_t which, int32_t value) {
    if (!h) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (which == HELLO_PILEUP_SHARE) {
        if (value < 0 || value > hello::kPileShare) return hello::set_last_error(HELLO_ERR_ARG, "share %d: 0 (sized by the launch) to %d", value, hello::kPileShare);
        h->share = value;
        return HELLO_OK;
    }
    if (which != HELLO_PILEUP_FORM) return hello::set_last_error(HELLO_ERR_ARG, "option %d", which);
    if (value != 0 && value != 1) return hello::set_last_error(HELLO_ERR_ARG, "form %d: 0 (two phases) or 1 (plain)", value);
    h->form = value;
    return HELLO_OK;
}

int hello_pileup_add(hello_pileup* h, const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                     const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                     const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads, int64_t lo, int64_t hi) try {
    using namespace hello;
    (void)hp;
    if (!h || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends || !mapq || !flags)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    h->check_span(lo, hi);

    // ---- the reads: validated, then the kernel's list
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    const std::vector<uint8_t> kind = pileup_walk(in, lo, h->mapq_threshold);
    std::vector<int64_t> list;
    int64_t n_belonging = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (!(kind[(size_t)r] & kPileBelongs)) continue;
        ++n_belonging;
        if (kind[(size_t)r] & kPileCounted) list.push_back(r);
    }
    const int64_t n_list = (int64_t)list.size();
    h->take_counting(n_list, kPileMaxReads, "counters");
    const int64_t share = h->share ? h->share : std::min<int64_t>(kPileShare, std::max<int64_t>(kPileWaves, (n_list + kPileGroups - 1) / kPileGroups));
    const int64_t n_blocks = (n_list + share - 1) / share;

    pile_build_sites(h);
    HS_HIP(hipSetDevice(h->device));
    std::vector<uint8_t> seen((size_t)n_list, 0);
    std::vector<unsigned long long> group_obs((size_t)n_blocks, 0);
    float reads_ms = 0.0f;
    if (n_list > 0 && h->n_sites > 0) {
        DevMem m;
        const DeviceReads d = upload_reads(m, in);
        PileReadsArgs a{};
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.ref_end = m.put(ref_ends, (size_t)n_reads);
        a.flags = m.put(flags, (size_t)n_reads);
        a.list = m.put(list.data(), list.size());
        a.seen = m.zeros<uint8_t>((size_t)n_list);
        a.n_list = n_list;
        a.sb = h->sb;
        a.q_threshold = h->q_threshold;
        a.share = (int)share;
        a.counts = h->counts.device;
        a.group_obs = m.room<unsigned long long>((size_t)n_blocks);
        KernelTimer timer;
        timer.start();
        if (h->form == 0) hipLaunchKernelGGL(pile_reads_kernel<true>, dim3((unsigned)n_blocks), dim3(kPileThreads), 0, 0, a);
        else hipLaunchKernelGGL(pile_reads_kernel<false>, dim3((unsigned)n_blocks), dim3(kPileThreads), 0, 0, a);
        reads_ms = timer.stop();
        h->counts.fetched = false;
        HS_HIP(hipMemcpy(seen.data(), a.seen, (size_t)n_list, hipMemcpyDeviceToHost));
        HS_HIP(hipMemcpy(group_obs.data(), a.group_obs, (size_t)n_blocks * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }

    // ---- nothing can fail from here on
    std::vector<uint8_t> status((size_t)n_reads, 0);
    int64_t n_on_a_site = 0;
    unsigned long long observations = 0;
    for (int64_t k = 0; k < n_list; ++k) {
        status[(size_t)list[(size_t)k]] = seen[(size_t)k] ? 2 : 1;
        n_on_a_site += seen[(size_t)k] ? 1 : 0;
    }
    for (unsigned long long v : group_obs) observations += v;
    h->status = std::move(status);
    h->counting_given += n_list;
    h->last_hi = hi;
    h->stats[0] += (double)n_reads;
    h->stats[1] += (double)n_belonging;
    h->stats[2] += (double)n_list;
    h->stats[3] += (double)n_on_a_site;
    h->stats[4] += (double)observations;
    h->stats[7] += reads_ms;
    return HELLO_OK;
} HS_ENTRY_END("hello_pileup_add")

int hello_pileup_array(hello_pileup* h, int32_t which, const void** data, int64_t* count) try {
    using namespace hello;
    if (!h || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    switch (which) {
        case HELLO_PILEUP_COUNTS:
            pile_build_sites(h);
            *data = h->counts.fetch(h->device).data(); *count = (int64_t)h->counts.host.size(); break;
        case HELLO_PILEUP_STATUS: *data = h->status.data(); *count = (int64_t)h->status.size(); break;
        default: return set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
} HS_ENTRY_END("hello_pileup_array")

int hello_pileup_stats(const hello_pileup* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    return h->copy_stats(stats);
}

void hello_pileup_free(hello_pileup* h) { delete h; }

static int contam_check_counts(const int64_t* const* arrays, int n_arrays, const double* af, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < n_arrays; ++k)
            if (arrays[k][i] < 0) return hello::set_last_error(HELLO_ERR_ARG, "site %lld: count %lld", (long long)i, (long long)arrays[k][i]);
        if (!(af[i] > 0.0 && af[i] < 1.0)) return hello::set_last_error(HELLO_ERR_ARG, "site %lld: AF %g is not inside (0, 1)", (long long)i, af[i]);
    }
    return HELLO_OK;
}

int hello_contam_estimate(const int64_t* r, const int64_t* a, const int64_t* o, const double* af, int64_t n, double* out) try {
    using namespace hello;
    if (!out || (n > 0 && (!r || !a || !o || !af))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    const int64_t* arrays[3] = {r, a, o};
    if (int rc = contam_check_counts(arrays, 3, af, n)) return rc;
    contam_estimate(r, a, o, af, n, out);
    return HELLO_OK;
} HS_ENTRY_END("hello_contam_estimate")

int hello_contam_identity(const int64_t* r1, const int64_t* a1, const int64_t* o1, const int64_t* r2, const int64_t* a2,
                          const int64_t* o2, const double* af, int64_t n, double* out) try {
    using namespace hello;
    if (!out || (n > 0 && (!r1 || !a1 || !o1 || !r2 || !a2 || !o2 || !af))) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    const int64_t* arrays[6] = {r1, a1, o1, r2, a2, o2};
    if (int rc = contam_check_counts(arrays, 6, af, n)) return rc;
    contam_identity(r1, a1, o1, r2, a2, o2, af, n, out);
    return HELLO_OK;
} HS_ENTRY_END("hello_contam_identity")

}  // extern "C"
