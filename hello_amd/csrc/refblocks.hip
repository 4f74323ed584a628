// Reference-confidence blocks of a gVCF (include/hello_mi355x.h: hello_refblocks_find): aligned reads + reference + the intervals
// the variant records cover -> the maximal runs of positions of one GQ band.  Not in the reference; DESIGN.md section 7f states
// the rules and hello_amd/gvcf.py restates them in Python, integer for integer.
//
// Host: the read filter, the validation of every counted read (the kernel reads within its bases), per source the counted reads in
// coordinate order with their running-max end, and per tile of kRbTile positions the contiguous range of each source's reads that
// can touch it and the sub-range of the excluded intervals.  Device, one workgroup per tile, two launches of one kernel:
//   count (WRITE = false): the four waves walk the tile's reads, one read per wave, CIGAR operation by operation (wave-uniform
//     loop, ended once the read has left the tile); the lanes take the positions of an M/=/X or D operation; n_total and n_ref are
//     integer LDS counters.  After a barrier the counters go to global memory, every position gets its key (excluded, no-call or
//     its GQ band), and the tile's number of runs is written.
//   write (WRITE = true): after an exclusive scan of the run counts on the host, the tile reloads its counters, forms the same
//     runs and writes each by index: the run's slots in LDS take the minimum of (GQ, position) and of the depth with integer
//     atomics, and the thread that owns the run's first position writes the record.
// The output capacity is exact, so no run can be dropped.  Counters are integers, minima are order-free and every record is written
// by its owner: two runs give the same bytes.  Runs of one key that meet at a tile edge are joined on the host.
#include <chrono>
#include <climits>
#include <cmath>
#include <memory>

#include "stage_host.h"

namespace hello {
namespace {

// Two int32 counters per position live in LDS, so a tile is four times kTile: 8 KB of counters, 8 KB of keys and GQs and 12 KB of
// run slots, 28 KB in all -- five workgroups (20 waves) fit the 160 KB of a CU, and a 150-base read is walked by (1024 + 150) /
// 1024 tiles on average where kTile walks it 1.6 times.  The packed (GQ, position) minimum needs kRbTile * 100 < 2^31.
constexpr int kRbTile = 1024;
constexpr int kRbThreads = 256;
constexpr int kRbPer = kRbTile / kRbThreads;
constexpr int kRbExcluded = -2;            // key of a position that belongs to no block

struct RbRun {
    int64_t start, end;
    int32_t band, min_dp, gq, n_ref, n_total, pad;
};

struct RbArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* list;         // the counted reads: source 0's in coordinate order, then source 1's
    const int64_t* list_end;     // reference end of list[k], from its CIGAR
    const int64_t* tile_reads;   // [tiles][4]: the ranges [b0, e0) and [b1, e1) of `list`
    const int64_t* tile_ex;      // [tiles][2]: the range of excluded intervals that can touch the tile
    const int64_t* ex_start;
    const int64_t* ex_stop;
    const uint8_t* ref;          // reference text of [lo, hi)
    int64_t lo, hi;
    int32_t* count_ref;          // [hi - lo]
    int32_t* count_total;
    int32_t* tile_runs;          // [tiles], written by the count launch
    const int64_t* run_off;      // [tiles], read by the write launch
    RbRun* runs;
    double a, b, c;              // -10 log10 of e, 1 - e and 0.5
    int q_threshold;
    int gq_binsize;
};

__device__ __forceinline__ double rb_pl(double l, double m) {
    const double v = floor((l - m) + 0.5);
    return v < 255.0 ? v : 255.0;
}

template <bool WRITE>
__global__ __launch_bounds__(kRbThreads) void refblocks_kernel(RbArgs a) {
    __shared__ int tot[kRbTile];
    __shared__ int nref[kRbTile];
    __shared__ int key[kRbTile];
    __shared__ int gqs[kRbTile];
    __shared__ int run_min[kRbTile];
    __shared__ int run_dp[kRbTile];
    __shared__ int run_end[kRbTile];
    __shared__ int wave_sum[kRbThreads / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x;
    const int64_t lo = a.lo + tile * kRbTile, hi = lo + kRbTile < a.hi ? lo + kRbTile : a.hi;
    const int n = (int)(hi - lo);

    if (!WRITE) {
        for (int j = tid; j < kRbTile; j += kRbThreads) { tot[j] = 0; nref[j] = 0; }
        __syncthreads();
        const int64_t b0 = a.tile_reads[4 * tile], n0 = a.tile_reads[4 * tile + 1] - b0;
        const int64_t b1 = a.tile_reads[4 * tile + 2], n1 = a.tile_reads[4 * tile + 3] - b1;
        for (int64_t k = wave; k < n0 + n1; k += kRbThreads / 64) {
            const int64_t at = k < n0 ? b0 + k : b1 + (k - n0);
            if (a.list_end[at] <= lo) continue;
            const int64_t r = a.list[at];
            const int64_t rs = a.ref_start[r];
            if (rs >= hi) continue;
            const uint8_t* bases = a.bases + a.read_off[r];
            const uint8_t* quals = a.quals + a.read_off[r];
            const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
            int64_t rf = rs, rd = 0;
            for (int64_t ci = 0; ci < n_ops && rf < hi; ++ci) {
                const unsigned c = a.cigars[c0 + ci];
                const int op = c & 15u;
                const int64_t len = c >> 4;
                if (op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF) {
                    int64_t nx = ci + 1;                                   // the next operation, skipping P
                    while (nx < n_ops && (a.cigars[c0 + nx] & 15u) == (unsigned)BAM_CPAD) ++nx;
                    const bool anchors = nx < n_ops && (a.cigars[c0 + nx] & 15u) == (unsigned)BAM_CINS;
                    const int64_t j0 = lo > rf ? lo - rf : 0, j1 = hi - rf < len ? hi - rf : len;
                    for (int64_t j = j0 + lane; j < j1; j += 64) {
                        const unsigned char u = bases[rd + j] & 0xDF;      // upper case of a letter
                        if (quals[rd + j] < a.q_threshold || !(u == 'A' || u == 'C' || u == 'G' || u == 'T')) continue;
                        const int64_t p = rf + j;
                        atomicAdd(&tot[p - lo], 1);
                        if ((a.ref[p - a.lo] & 0xDF) == u && !(anchors && j == len - 1)) atomicAdd(&nref[p - lo], 1);
                    }
                    rf += len;
                    rd += len;
                } else if (op == BAM_CDEL) {
                    const int64_t j0 = lo > rf ? lo - rf : 0, j1 = hi - rf < len ? hi - rf : len;
                    for (int64_t j = j0 + lane; j < j1; j += 64) atomicAdd(&tot[rf + j - lo], 1);
                    rf += len;
                } else if (op == BAM_CREF_SKIP) {
                    rf += len;
                } else if (op == BAM_CINS || op == BAM_CSOFT_CLIP) {
                    rd += len;
                }
            }
        }
        __syncthreads();
        for (int j = tid; j < n; j += kRbThreads) {
            a.count_total[lo - a.lo + j] = tot[j];
            a.count_ref[lo - a.lo + j] = nref[j];
        }
    } else {
        for (int j = tid; j < kRbTile; j += kRbThreads) {
            tot[j] = j < n ? a.count_total[lo - a.lo + j] : 0;
            nref[j] = j < n ? a.count_ref[lo - a.lo + j] : 0;
        }
        __syncthreads();
    }

    // ---- the key of every position: excluded, no-call or the GQ band
    const int64_t eb = a.tile_ex[2 * tile], ee = a.tile_ex[2 * tile + 1];
    for (int j = tid; j < kRbTile; j += kRbThreads) {
        int k = kRbExcluded, g = 0;
        if (j < n) {
            const int64_t p = lo + j;
            int64_t x = eb, y = ee;                                        // the last interval that starts at or before p
            while (x < y) {
                const int64_t mid = (x + y) >> 1;
                if (a.ex_start[mid] <= p) x = mid + 1; else y = mid;
            }
            if (!(x > eb && p < a.ex_stop[x - 1])) {
                const int t = tot[j], r = nref[j];
                const double nt = (double)t, nr = (double)r, na = (double)(t - r);
                const double l00 = a.a * na + a.b * nr, l01 = a.c * nt, l11 = a.a * nr + a.b * na;
                const double m = fmin(l00, fmin(l01, l11));
                k = HELLO_REFBLOCKS_NO_CALL;
                if (l00 < l01 && l00 < l11) {
                    const double q = fmin(99.0, fmin(rb_pl(l01, m), rb_pl(l11, m)));
                    g = (int)q;
                    k = g / a.gq_binsize;
                }
            }
        }
        key[j] = k;
        gqs[j] = g;
        run_min[j] = INT_MAX;
        run_dp[j] = INT_MAX;
        run_end[j] = 0;
    }
    __syncthreads();

    // ---- runs inside the tile: a run starts where the key changes; thread t owns positions [kRbPer t, kRbPer (t + 1))
    bool starts[kRbPer];
    int mine = 0;
    for (int i = 0; i < kRbPer; ++i) {
        const int j = tid * kRbPer + i;
        starts[i] = key[j] != kRbExcluded && (j == 0 || key[j - 1] != key[j]);
        mine += starts[i] ? 1 : 0;
    }
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
    for (int w = 0; w < kRbThreads / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    if (!WRITE) {
        if (tid == 0) a.tile_runs[tile] = total;
        return;
    }
    int index[kRbPer];
    int ri = before - 1;
    for (int i = 0; i < kRbPer; ++i) {
        const int j = tid * kRbPer + i;
        if (starts[i]) ++ri;
        index[i] = ri;
        if (key[j] == kRbExcluded) continue;                              // ri >= 0: a run started at or before j
        atomicMin(&run_min[ri], gqs[j] * kRbTile + j);                    // the smallest GQ, at its first position
        atomicMin(&run_dp[ri], tot[j]);
        atomicMax(&run_end[ri], j + 1);
    }
    __syncthreads();
    for (int i = 0; i < kRbPer; ++i) {
        if (!starts[i]) continue;
        const int j = tid * kRbPer + i, r = index[i], at = run_min[r] % kRbTile;
        RbRun out;
        out.start = lo + j;
        out.end = lo + run_end[r];
        out.band = key[j];
        out.min_dp = run_dp[r];
        out.gq = run_min[r] / kRbTile;
        out.n_ref = nref[at];
        out.n_total = tot[at];
        out.pad = 0;
        a.runs[a.run_off[tile] + r] = out;
    }
}

}  // namespace
}  // namespace hello

struct hello_refblocks {
    std::vector<int64_t> start, end;
    std::vector<int32_t> band, min_dp, gq, n_ref, n_total, count_ref, count_total;
    double stats[HELLO_REFBLOCKS_STATS] = {0};
};

extern "C" {

int hello_refblocks_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                         const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                         const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                         const uint8_t* reference, int64_t reference_length, int64_t lo, int64_t hi, const int64_t* excluded_starts,
                         const int64_t* excluded_stops, int64_t n_excluded, int32_t q_threshold, int32_t mapq_threshold,
                         int32_t gq_binsize, int32_t options, int32_t device, hello_refblocks** out) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!out || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends ||
        !mapq || !flags || !name_hash || !source)) || !reference || (n_excluded > 0 && (!excluded_starts || !excluded_stops)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    if (n_reads < 0 || n_excluded < 0 || reference_length < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    if (lo < 0 || hi < lo || hi > reference_length)
        return set_last_error(HELLO_ERR_ARG, "span [%lld, %lld) of a reference of %lld bases", (long long)lo, (long long)hi,
                              (long long)reference_length);
    if (gq_binsize < 1) return set_last_error(HELLO_ERR_ARG, "gq_binsize %d: at least 1", gq_binsize);
    if (options & ~HELLO_REFBLOCKS_KEEP_COUNTS) return set_last_error(HELLO_ERR_ARG, "options %d", options);
    for (int64_t i = 0; i < n_excluded; ++i)
        if (excluded_starts[i] > excluded_stops[i] || (i > 0 && excluded_starts[i] < excluded_stops[i - 1]))
            return set_last_error(HELLO_ERR_ARG, "excluded interval %lld: [%lld, %lld) is not sorted behind its predecessor",
                                  (long long)i, (long long)excluded_starts[i], (long long)excluded_stops[i]);

    // ---- the counted reads of each source, validated: the kernel reads within their bases
    std::vector<int64_t> list[2], list_end[2], max_end[2], starts[2];
    int64_t last_start[2] = {INT64_MIN, INT64_MIN};
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    for (int64_t r = 0; r < n_reads; ++r) {
        const int s = source[r];
        if (s > 1) return set_last_error(HELLO_ERR_ARG, "source[%lld] = %d: 0 or 1", (long long)r, s);
        if (ref_starts[r] < last_start[s])
            return set_last_error(HELLO_ERR_ARG, "read %lld: reads are not coordinate-sorted (the BAM must be)", (long long)r);
        last_start[s] = ref_starts[r];
        int64_t qlen, rlen;
        if (!counted_walk(in, r, mapq_threshold, qlen, rlen)) continue;
        const int64_t end = ref_starts[r] + rlen;
        if (end <= lo || ref_starts[r] >= hi) continue;
        list[s].push_back(r);
        list_end[s].push_back(end);
        starts[s].push_back(ref_starts[r]);
        max_end[s].push_back(max_end[s].empty() ? end : std::max(max_end[s].back(), end));
    }

    // ---- tiles: per source the contiguous range from the first read whose running-max end exceeds the tile's low edge to the
    // last read that starts below its high edge; the excluded intervals that can touch the tile
    const int64_t span = hi - lo, n_tiles = (span + kRbTile - 1) / kRbTile;
    if (n_tiles > INT32_MAX) return set_last_error(HELLO_ERR_ARG, "span of %lld positions", (long long)span);
    std::vector<int64_t> tile_reads((size_t)n_tiles * 4), tile_ex((size_t)n_tiles * 2);
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t tl = lo + t * kRbTile, th = std::min(tl + kRbTile, hi);
        int64_t base = 0;
        for (int s = 0; s < 2; ++s) {
            const int64_t b = std::upper_bound(max_end[s].begin(), max_end[s].end(), tl) - max_end[s].begin();
            const int64_t e = std::lower_bound(starts[s].begin(), starts[s].end(), th) - starts[s].begin();
            tile_reads[4 * t + 2 * s] = base + b;
            tile_reads[4 * t + 2 * s + 1] = base + std::max(b, e);
            base += (int64_t)list[s].size();
        }
        const int64_t eb = std::upper_bound(excluded_stops, excluded_stops + n_excluded, tl) - excluded_stops;
        const int64_t ee = std::lower_bound(excluded_starts, excluded_starts + n_excluded, th) - excluded_starts;
        tile_ex[2 * t] = eb;
        tile_ex[2 * t + 1] = std::max(eb, ee);
    }
    list[0].insert(list[0].end(), list[1].begin(), list[1].end());
    list_end[0].insert(list_end[0].end(), list_end[1].begin(), list_end[1].end());
    const int64_t counted = (int64_t)list[0].size();
    const auto t1 = clock::now();

    auto* res = new hello_refblocks();
    std::unique_ptr<hello_refblocks> own(res);
    float kernel_ms = 0.0f;
    int64_t n_runs = 0;
    if (n_tiles > 0) {
        open_device(device);
        DevMem m;
        RbArgs a{};
        const DeviceReads d = upload_reads(m, in);
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.list = m.put(list[0].data(), list[0].size());
        a.list_end = m.put(list_end[0].data(), list_end[0].size());
        a.tile_reads = m.put(tile_reads.data(), tile_reads.size());
        a.tile_ex = m.put(tile_ex.data(), tile_ex.size());
        a.ex_start = m.put(excluded_starts, (size_t)n_excluded);
        a.ex_stop = m.put(excluded_stops, (size_t)n_excluded);
        a.ref = m.put(reference + lo, (size_t)span);
        a.lo = lo;
        a.hi = hi;
        a.count_ref = m.zeros<int32_t>((size_t)span);
        a.count_total = m.zeros<int32_t>((size_t)span);
        a.tile_runs = m.zeros<int32_t>((size_t)n_tiles);
        const double e = 0.001;
        a.a = -10.0 * std::log10(e);
        a.b = -10.0 * std::log10(1.0 - e);
        a.c = -10.0 * std::log10(0.5);
        a.q_threshold = q_threshold;
        a.gq_binsize = gq_binsize;
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(refblocks_kernel<false>, dim3((unsigned)n_tiles), dim3(kRbThreads), 0, 0, a);
        kernel_ms += timer.stop();
        std::vector<int32_t> tile_runs((size_t)n_tiles);
        HS_HIP(hipMemcpy(tile_runs.data(), a.tile_runs, tile_runs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<int64_t> run_off((size_t)n_tiles);
        for (int64_t t = 0; t < n_tiles; ++t) {                              // exclusive scan: the capacity is exact
            if (tile_runs[t] < 0 || tile_runs[t] > kRbTile) raise(HELLO_ERR_HIP, "tile %lld reports %d runs", (long long)t, tile_runs[t]);
            run_off[t] = n_runs;
            n_runs += tile_runs[t];
        }
        a.run_off = m.put(run_off.data(), run_off.size());
        a.runs = m.zeros<RbRun>((size_t)n_runs);
        timer.start();
        hipLaunchKernelGGL(refblocks_kernel<true>, dim3((unsigned)n_tiles), dim3(kRbThreads), 0, 0, a);
        kernel_ms += timer.stop();
        std::vector<RbRun> runs((size_t)n_runs);
        if (n_runs) HS_HIP(hipMemcpy(runs.data(), a.runs, runs.size() * sizeof(RbRun), hipMemcpyDeviceToHost));
        if (options & HELLO_REFBLOCKS_KEEP_COUNTS) {
            res->count_ref.resize((size_t)span);
            res->count_total.resize((size_t)span);
            HS_HIP(hipMemcpy(res->count_ref.data(), a.count_ref, (size_t)span * sizeof(int32_t), hipMemcpyDeviceToHost));
            HS_HIP(hipMemcpy(res->count_total.data(), a.count_total, (size_t)span * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        // ---- runs of one key that meet at a tile edge are one block: the smaller GQ wins, the earlier position on a tie
        for (const RbRun& r : runs) {
            if (!res->start.empty() && res->end.back() == r.start && res->band.back() == r.band) {
                res->end.back() = r.end;
                res->min_dp.back() = std::min(res->min_dp.back(), r.min_dp);
                if (r.gq < res->gq.back()) {
                    res->gq.back() = r.gq;
                    res->n_ref.back() = r.n_ref;
                    res->n_total.back() = r.n_total;
                }
                continue;
            }
            res->start.push_back(r.start);
            res->end.push_back(r.end);
            res->band.push_back(r.band);
            res->min_dp.push_back(r.min_dp);
            res->gq.push_back(r.gq);
            res->n_ref.push_back(r.n_ref);
            res->n_total.push_back(r.n_total);
        }
    }
    const double ms_plan = std::chrono::duration<double, std::milli>(t1 - t0).count();
    const double ms_total = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    const double st[HELLO_REFBLOCKS_STATS] = {(double)n_tiles, (double)counted, (double)n_runs, (double)res->start.size(), kernel_ms,
                                              ms_plan, ms_total};
    std::copy(st, st + HELLO_REFBLOCKS_STATS, res->stats);
    *out = own.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_refblocks_find")

int hello_refblocks_array(const hello_refblocks* h, int32_t which, const void** data, int64_t* count) {
    if (!h || !data || !count) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    switch (which) {
        case HELLO_REFBLOCKS_START: *data = h->start.data(); *count = (int64_t)h->start.size(); break;
        case HELLO_REFBLOCKS_END: *data = h->end.data(); *count = (int64_t)h->end.size(); break;
        case HELLO_REFBLOCKS_BAND: *data = h->band.data(); *count = (int64_t)h->band.size(); break;
        case HELLO_REFBLOCKS_MIN_DP: *data = h->min_dp.data(); *count = (int64_t)h->min_dp.size(); break;
        case HELLO_REFBLOCKS_GQ: *data = h->gq.data(); *count = (int64_t)h->gq.size(); break;
        case HELLO_REFBLOCKS_N_REF: *data = h->n_ref.data(); *count = (int64_t)h->n_ref.size(); break;
        case HELLO_REFBLOCKS_N_TOTAL: *data = h->n_total.data(); *count = (int64_t)h->n_total.size(); break;
        case HELLO_REFBLOCKS_COUNT_REF: *data = h->count_ref.data(); *count = (int64_t)h->count_ref.size(); break;
        case HELLO_REFBLOCKS_COUNT_TOTAL: *data = h->count_total.data(); *count = (int64_t)h->count_total.size(); break;
        default: return hello::set_last_error(HELLO_ERR_ARG, "array selector %d", which);
    }
    return HELLO_OK;
}

int hello_refblocks_stats(const hello_refblocks* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_REFBLOCKS_STATS, stats);
    return HELLO_OK;
}

void hello_refblocks_free(hello_refblocks* h) { delete h; }

}  // extern "C"
