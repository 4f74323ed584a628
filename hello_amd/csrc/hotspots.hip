// Candidate-position detector (include/hello_mi355x.h: hello_hotspots_find): aligned reads + reference -> the sorted positions
// the reference's hotspot stage writes.
//
// Reference semantics: python/HotspotDetectorDVFiltered.py:14-15,31-165 (chunks, one searcher per chunk, clipping, union),
// python/PileupContainerLite.py:526-570 and python/PileupContainer.py:33-41 (the read set of a chunk), python/AlleleSearcherLite.py:
// 112-160,187-205 (the window and its bounds), c++/src/AlleleSearcherLiteFiltered.cpp:121-317 (counting), :19-100 (partial
// insertions), :834-890 and :550-609 (flagging, :611-646 choosing between them).  DESIGN.md "Candidate positions" restates the rules.
//
// Host: the chunk plan (read filters, de-duplication, the read cap, the window bounds that skip a chunk) and, per chunk, tiles of
// kTile genome positions over the span its counted reads touch.  Device: the counting, partial-resolution and flagging kernel of
// differing.h (shared with candidates.hip), one workgroup per tile; here a chunk's flags are clipped to the chunk and its bits sit
// at the chunk's offset in one bitmap over the regions' span.
#include <chrono>
#include <memory>
#include <unordered_set>

#include "differing.h"
#include "stage_host.h"

struct hello_hotspots {
    std::vector<int64_t> positions;
    double stats[HELLO_HOTSPOTS_STATS] = {0};
};

extern "C" {

int hello_hotspots_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                        const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                        const uint16_t* flags, const uint64_t* name_hash, const uint8_t* source, int64_t n_reads,
                        const uint8_t* reference, int64_t reference_length, const int64_t* region_starts,
                        const int64_t* region_stops, int32_t n_regions, int32_t options, int32_t q_threshold,
                        int32_t mapq_threshold, int32_t device, hello_hotspots** out) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!out || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends ||
        !mapq || !flags || !name_hash || !source)) || !reference || (n_regions > 0 && (!region_starts || !region_stops)))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    if (n_reads < 0 || n_regions < 0 || reference_length < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    // the number of read sets is the caller's (a second BAM without reads in the region still means 10 kbp chunks)
    const bool two = (options & HELLO_HOTSPOTS_TWO_BAMS) != 0;
    const bool pacbio = (options & HELLO_HOTSPOTS_PACBIO) != 0, hybrid = (options & HELLO_HOTSPOTS_HYBRID) != 0;
    if (two && pacbio) return set_last_error(HELLO_ERR_ARG, "HELLO_HOTSPOTS_PACBIO describes one read set; two were given");
    // HotspotDetectorDVFiltered.py:14-17,189-215,227-254: chunk sizes and read caps per read set; two read sets share 10 kbp chunks
    const int64_t chunk_size = (two || pacbio) ? 10000 : 400;
    const int64_t cap[2] = {pacbio ? 1000 : 10000, 1000};
    const uint8_t table_of[2] = {(uint8_t)(pacbio ? 1 : 0), 1};

    // ---- validation of every usable read: the kernel reads within its bases and within the reference
    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    ReadLayout layout;                                       // planting positions (pos - 1) of every I/D operation of a usable read
    strict_walk(in, kStrictPlain, layout, nullptr, source, two ? 2 : 1);
    const std::vector<int64_t>& plant_off = layout.plant_off;
    const std::vector<int64_t>& plant = layout.plant;
    const int64_t* max_span = layout.max_span;
    std::vector<int64_t> order[2];
    for (int64_t r = 0; r < n_reads; ++r) order[source[r]].push_back(r);

    // ---- chunk plan
    auto* res = new hello_hotspots();
    std::unique_ptr<hello_hotspots> own(res);
    std::vector<int64_t> cbeg, cend, creads_off{0}, creads, tile_lo, tile_ev_off{0};
    std::vector<int32_t> tile_chunk;
    int64_t span_lo = INT64_MAX, span_hi = INT64_MIN, ref_lo = INT64_MAX, ref_hi = INT64_MIN;
    int64_t n_chunks = 0, n_empty = 0, n_bounds = 0, n_capped = 0;
    std::vector<int64_t> kept[2];
    std::unordered_set<std::pair<uint64_t, int>, PairHash> seen;
    for (int32_t g = 0; g < n_regions; ++g) {
        const int64_t rs = region_starts[g], re = region_stops[g];
        if (rs < 0 || re < rs) return set_last_error(HELLO_ERR_ARG, "region %d: [%lld, %lld)", g, (long long)rs, (long long)re);
        if (re > rs) { span_lo = std::min(span_lo, rs); span_hi = std::max(span_hi, re); }
        for (int64_t b = rs; b < re; b += chunk_size) {             // :110-112 numChunks = ceil((stop - start) / chunkSize)
            const int64_t e = std::min(b + chunk_size, re);
            ++n_chunks;
            bool capped = false;
            for (int s = 0; s < 2; ++s) {                            // PileupContainerLite.__get_reads (:526-570)
                kept[s].clear();
                seen.clear();
                const auto& o = order[s];
                auto it = std::lower_bound(o.begin(), o.end(), b - max_span[s],
                                           [&](int64_t r, int64_t v) { return ref_starts[r] < v; });
                for (; it != o.end() && ref_starts[*it] < e; ++it) {
                    const int64_t r = *it;
                    if (ref_ends[r] <= b || !usable(flags[r], mapq[r])) continue;
                    if (!seen.insert({name_hash[r], (flags[r] & 16) ? 1 : 0}).second) continue;
                    if ((int64_t)kept[s].size() >= cap[s]) { capped = true; continue; }
                    kept[s].push_back(r);
                }
            }
            if (kept[0].empty() && kept[1].empty()) { ++n_empty; continue; }            // doOneChunk :84-85
            n_capped += capped;
            int64_t ws = b, we = INT64_MIN;                                              // AlleleSearcherLite.py:137-151
            for (int s = 0; s < 2; ++s)
                for (int64_t r : kept[s]) { ws = std::min(ws, ref_starts[r]); we = std::max(we, ref_ends[r]); }
            ws -= 10;
            if (ws < 0 || we > reference_length) { ++n_bounds; continue; }
            const int32_t chunk = (int32_t)cbeg.size();
            cbeg.push_back(b);
            cend.push_back(e);
            int64_t lo0 = INT64_MAX, hi0 = INT64_MIN;
            const size_t first = creads.size();
            for (int s = 0; s < 2; ++s)
                for (int64_t r : kept[s])
                    if (mapq[r] >= mapq_threshold) {                                     // :134-136
                        creads.push_back(r);
                        lo0 = std::min(lo0, ref_starts[r] - 1);
                        hi0 = std::max(hi0, ref_ends[r]);
                    }
            creads_off.push_back((int64_t)creads.size());
            if (creads.size() == first) continue;
            ref_lo = std::min(ref_lo, lo0);
            ref_hi = std::max(ref_hi, hi0);
            const int64_t nt = (hi0 - lo0 + kTile - 1) / kTile;
            std::vector<int64_t> capacity(nt, 0);
            for (size_t k = first; k < creads.size(); ++k) {
                const int64_t r = creads[k];                             // each I/D lands in the one tile of its planting position
                for (int64_t i = plant_off[r]; i < plant_off[r + 1]; ++i) ++capacity[(plant[i] - lo0) / kTile];
            }
            for (int64_t t = 0; t < nt; ++t) {
                tile_chunk.push_back(chunk);
                tile_lo.push_back(lo0 + t * kTile);
                tile_ev_off.push_back(tile_ev_off.back() + capacity[t]);
            }
        }
    }
    std::vector<uint8_t> table(n_reads);
    for (int64_t r = 0; r < n_reads; ++r) table[r] = table_of[source[r]];
    const auto t1 = clock::now();

    const int64_t n_tiles = (int64_t)tile_lo.size();
    float kernel_ms = 0.0f;
    if (n_tiles > 0) {
        open_device(device);
        DevMem m;
        HotspotArgs a{};
        const DeviceReads d = upload_reads(m, in);
        a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
        a.ref_start = d.ref_start;
        a.ref_end = m.put(ref_ends, (size_t)n_reads);
        a.table = m.put(table.data(), table.size());
        a.chunk_reads = m.put(creads.data(), creads.size());
        a.chunk_reads_off = m.put(creads_off.data(), creads_off.size());
        std::vector<int64_t> bit_base(cbeg.size());
        for (size_t c = 0; c < cbeg.size(); ++c) bit_base[c] = cbeg[c] - span_lo;   // bit i: position span_lo + i flagged
        a.flag_lo = m.put(cbeg.data(), cbeg.size());
        a.flag_hi = m.put(cend.data(), cend.size());
        a.bit_base = m.put(bit_base.data(), bit_base.size());
        a.tile_chunk = m.put(tile_chunk.data(), tile_chunk.size());
        a.tile_lo = m.put(tile_lo.data(), tile_lo.size());
        a.tile_ev_off = m.put(tile_ev_off.data(), tile_ev_off.size());
        a.events = m.zeros<HsEvent>((size_t)tile_ev_off.back());
        a.ref_lo = ref_lo;
        a.ref_len = ref_hi - ref_lo;
        a.ref = m.put(reference + ref_lo, (size_t)a.ref_len);
        const int64_t words = (span_hi - span_lo + 31) / 32;
        a.bitmap = m.zeros<unsigned>((size_t)words);
        a.q_threshold = q_threshold;
        a.hybrid = hybrid ? 1 : 0;
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(hotspot_kernel, dim3((unsigned)n_tiles), dim3(256), 0, 0, a);
        kernel_ms = timer.stop();
        std::vector<unsigned> bits((size_t)words);
        HS_HIP(hipMemcpy(bits.data(), a.bitmap, bits.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (int64_t w = 0; w < words; ++w)
            for (unsigned v = bits[w]; v; v &= v - 1) res->positions.push_back(span_lo + 32 * w + __builtin_ctz(v));
    }
    const int64_t counted = (int64_t)creads.size();
    const double ms_plan = std::chrono::duration<double, std::milli>(t1 - t0).count();
    const double ms_total = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    const double st[HELLO_HOTSPOTS_STATS] = {(double)n_chunks, (double)n_empty, (double)n_bounds, (double)n_capped, (double)counted,
                                             (double)n_tiles, (double)tile_ev_off.back(), kernel_ms, ms_plan, ms_total};
    std::copy(st, st + HELLO_HOTSPOTS_STATS, res->stats);
    *out = own.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_hotspots_find")

int hello_hotspots_positions(const hello_hotspots* h, const int64_t** positions, int64_t* n_positions) {
    if (!h || !positions || !n_positions) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *positions = h->positions.data();
    *n_positions = (int64_t)h->positions.size();
    return HELLO_OK;
}

int hello_hotspots_stats(const hello_hotspots* h, double* stats) {
    if (!h || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(h->stats, h->stats + HELLO_HOTSPOTS_STATS, stats);
    return HELLO_OK;
}

void hello_hotspots_free(hello_hotspots* h) { delete h; }

}  // extern "C"
