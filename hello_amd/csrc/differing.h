// Differing positions of a set of reads against the reference: the counting, partial-resolution and flagging kernel that the
// hotspot stage (hotspots.hip) and the candidate stage (candidates.hip) share; the host layer is stage_host.h.  A "chunk" is any
// region with its own read list; the kernel keeps the flagged positions of a chunk on [flag_lo, flag_hi) in the chunk's own bits.
//
// Device: one workgroup per tile of kTile genome positions.  Its four waves walk the chunk's reads, one read per wave, CIGAR
// operation by operation (wave-uniform loop, as featurize_kernel does); the lanes take the bases of an M/=/X operation.
// Per-position integer counts -- `total` and one SNV count per read base code, per technology table -- live in LDS; insertions
// and deletions go to the tile's event list in global memory, whose capacity the host counted exactly (the I/D operations of the
// chunk's counted reads whose planting position, pos - 1, lies in the tile).  After a barrier the same workgroup resolves the
// partial insertions against the distinct full keys of their position (string compares), adds the resolved counts, applies the
// float32 thresholds of the reference, and sets the flagged positions in a bitmap with atomicOr.  All counts are integers and the
// bitmap is an OR, so the result does not depend on the order of any atomic: two runs give the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "cigar.h"

namespace hello {
namespace {

constexpr int kTile = 256;                 // genome positions per workgroup
constexpr int kCodes = 16;                 // BAM read base codes "=ACMGRSVTWYHKDBN"
constexpr int kFull = 0, kLeft = 1, kRight = 2;

struct HsEvent {
    int64_t alt_off;     // index into `bases` of the alt's first read byte
    int32_t pos;         // tile-relative position the event is planted at
    int32_t ref_len;     // reference allele = ref[pos, pos + ref_len)
    int32_t alt_len;     // read bytes of the alt allele
    int32_t inc;         // 2 for Illumina, 1 for PacBio (:234,262,280,301)
    int32_t target;      // partials: -1 unresolved, >= 0 the event holding the matched full key, -2 - c the SNV key of code c
    uint8_t table;       // 0 Illumina counts (counts_i), 1 PacBio counts (counts_p)
    uint8_t kind;        // kFull | kLeft | kRight
    uint8_t lead;        // the alt starts with ref[pos] (a deletion or insertion at the read's first base, :223,289)
    uint8_t rep;         // full events: first of its key in the list (the distinct keys of :36-57)
};

struct HotspotArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const int64_t* ref_end;
    const uint8_t* table;            // per read
    const int64_t* chunk_reads;      // counted reads of every chunk, concatenated
    const int64_t* chunk_reads_off;  // [chunks + 1]
    const int64_t* flag_lo;          // per chunk: flagged positions are kept on [flag_lo, flag_hi) ...
    const int64_t* flag_hi;
    const int64_t* bit_base;         // ... and position p of the chunk is bit bit_base + p - flag_lo of the bitmap
    const int32_t* tile_chunk;
    const int64_t* tile_lo;          // genome position of the tile's first column
    const int64_t* tile_ev_off;      // [tiles + 1] event capacity offsets
    HsEvent* events;
    const uint8_t* ref;              // reference text of [ref_lo, ref_lo + ref_len)
    int64_t ref_lo, ref_len;
    unsigned* bitmap;
    int q_threshold;
    int hybrid;
};

__device__ __forceinline__ int base_code(unsigned char b) {
    switch (b) {
        case '=': return 0;  case 'A': return 1;  case 'C': return 2;  case 'M': return 3;
        case 'G': return 4;  case 'R': return 5;  case 'S': return 6;  case 'V': return 7;
        case 'T': return 8;  case 'W': return 9;  case 'Y': return 10; case 'H': return 11;
        case 'K': return 12; case 'D': return 13; case 'B': return 14; default: return 15;
    }
}
__device__ const char kCodeBase[17] = "=ACMGRSVTWYHKDBN";

__global__ __launch_bounds__(256) void hotspot_kernel(HotspotArgs a) {
    __shared__ int tot[2][kTile];
    __shared__ int snv[2][kTile][kCodes];
    __shared__ int n_ev;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = blockIdx.x;
    const int chunk = a.tile_chunk[tile];
    const int64_t lo = a.tile_lo[tile], hi = lo + kTile;
    for (int i = tid; i < 2 * kTile; i += 256) (&tot[0][0])[i] = 0;
    for (int i = tid; i < 2 * kTile * kCodes; i += 256) (&snv[0][0][0])[i] = 0;
    if (tid == 0) n_ev = 0;
    __syncthreads();

    HsEvent* ev = a.events + a.tile_ev_off[tile];
    const int cap = (int)(a.tile_ev_off[tile + 1] - a.tile_ev_off[tile]);
    auto ref_at = [&](int64_t p) -> unsigned char {                 // the planner keeps every p inside; 0 mismatches all bases
        const int64_t i = p - a.ref_lo;
        return (i >= 0 && i < a.ref_len) ? a.ref[i] : (unsigned char)0;
    };
    auto emit = [&](int kind, int t, int64_t p, int ref_len, int64_t alt_off, int alt_len, int lead) {
        const int slot = atomicAdd(&n_ev, 1);
        if (slot >= cap) return;                                   // cannot happen: the capacity counts every I/D planted here
        HsEvent e;
        e.alt_off = alt_off; e.pos = (int32_t)(p - lo); e.ref_len = ref_len; e.alt_len = alt_len;
        e.inc = t ? 1 : 2; e.target = -1; e.table = (uint8_t)t; e.kind = (uint8_t)kind; e.lead = (uint8_t)lead; e.rep = 0;
        ev[slot] = e;
    };

    // ---- counting: AlleleSearcherLiteFiltered::updateAlleleCounts (:121-317), one wave per read
    for (int64_t k = a.chunk_reads_off[chunk] + wave; k < a.chunk_reads_off[chunk + 1]; k += 4) {
        const int64_t r = a.chunk_reads[k];
        const int64_t rs = a.ref_start[r];
        if (rs - 1 >= hi || a.ref_end[r] <= lo) continue;         // plants only into [rs - 1, ref_end)
        const int t = a.table[r];
        const int64_t roff = a.read_off[r];
        const uint8_t* bases = a.bases + roff;
        const uint8_t* quals = a.quals + roff;
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = rs, rd = 0;
        for (int64_t ci = 0; ci < n_ops && rf - 1 < hi; ++ci) {   // nothing after rf - 1 >= hi lands in this tile
            const unsigned c = a.cigars[c0 + ci];
            const int op = c & 15u;
            const int64_t len = c >> 4;
            if (op == BAM_CMATCH || op == BAM_CEQUAL || op == BAM_CDIFF) {          // :184-216
                const int64_t j0 = lo > rf ? lo - rf : 0, j1 = hi - rf < len ? hi - rf : len;
                for (int64_t j = j0 + lane; j < j1; j += 64) {
                    const int64_t p = rf + j;
                    const unsigned char b = bases[rd + j], rb = ref_at(p);
                    if (b != rb && quals[rd + j] >= a.q_threshold && b != 'N' && rb != 'N')  // :192-197, :155-162
                        atomicAdd(&snv[t][p - lo][base_code(b)], 1);
                    atomicAdd(&tot[t][p - lo], 1);                                     // :202
                }
                rf += len;
                rd += len;
            } else if (op == BAM_CDEL) {                                               // :218-238, falls through to :239-243
                const int64_t p = rf - 1;
                if (lane == 0 && p >= lo && p < hi) {
                    bool ok = rd == 0 || quals[rd - 1] >= a.q_threshold;               // rdcounter - 1 < 0: no check (:158)
                    const unsigned char alt = rd > 0 ? bases[rd - 1] : ref_at(p);
                    ok = ok && alt != 'N';
                    for (int64_t i = p; ok && i <= rf + len - 1; ++i) ok = ref_at(i) != 'N';
                    if (ok) emit(kFull, t, p, (int)(len + 1), rd > 0 ? roff + rd - 1 : roff, rd > 0 ? 1 : 0, rd > 0 ? 0 : 1);
                }
                rf += len;
            } else if (op == BAM_CREF_SKIP) {                                          // :239-243
                rf += len;
            } else if (op == BAM_CINS) {                                               // :245-304, falls through to :305-309
                const int64_t p = rf - 1;
                if (lane == 0 && p >= lo && p < hi) {
                    int kind = kFull, lead = 0;
                    int64_t s, n;
                    if (ci == 0) {                                   // left partial: cigarcount counts hard clips too (:250)
                        kind = kLeft; s = rd; n = len;
                        atomicAdd(&tot[t][p - lo], 1);               // :267, whatever the quality
                    } else if (ci == n_ops - 1 && rd > 0) {          // right partial (:268)
                        kind = kRight; s = rd - 1; n = len + 1;
                    } else if (rd > 0) {
                        s = rd - 1; n = len + 1;
                    } else {                                         // refAllele + read bases (:289), quality over the read part
                        s = 0; n = len; lead = 1;
                    }
                    int qmin = 255;
                    bool ok = ref_at(p) != 'N';
                    for (int64_t i = s; i < s + n; ++i) {
                        qmin = quals[i] < qmin ? quals[i] : qmin;
                        ok = ok && bases[i] != 'N';
                    }
                    if (ok && qmin >= a.q_threshold) emit(kind, t, p, 1, roff + s, (int)n, lead);
                }
                rd += len;
            } else if (op == BAM_CSOFT_CLIP) {                                         // :305-309
                rd += len;
            }
        }
    }
    __syncthreads();
    const int E = n_ev < cap ? n_ev : cap;

    auto alt_size = [&](const HsEvent& e) { return e.alt_len + e.lead; };
    auto alt_char = [&](const HsEvent& e, int i) -> unsigned char {
        return (e.lead && i == 0) ? ref_at(lo + e.pos) : a.bases[e.alt_off + i - e.lead];
    };
    auto same_key = [&](const HsEvent& x, const HsEvent& y) {       // (refAllele, altAllele) at one position
        if (x.pos != y.pos || x.ref_len != y.ref_len || alt_size(x) != alt_size(y)) return false;
        for (int i = 0; i < alt_size(x); ++i)
            if (alt_char(x, i) != alt_char(y, i)) return false;
        return true;
    };

    // ---- distinct full keys
    for (int f = tid; f < E; f += 256) {
        const HsEvent e = ev[f];
        if (e.kind != kFull) continue;
        bool first = true;
        for (int g = 0; g < f && first; ++g) {
            const HsEvent o = ev[g];
            if (o.kind == kFull && o.table == e.table && same_key(o, e)) first = false;
        }
        ev[f].rep = first ? 1 : 0;
    }
    __syncthreads();

    // ---- AlleleCounts::resolvePartials (:19-100): a partial matches a key whose alt ends (left) / starts (right) with its alt;
    // exactly one matching key takes its count, otherwise it is dropped.  Matching never depends on counts, so the left and the
    // right pass resolve independently.
    for (int pi = tid; pi < E; pi += 256) {
        const HsEvent p = ev[pi];
        if (p.kind == kFull) continue;
        const int plen = alt_size(p);
        int matches = 0, target = -1;
        for (int f = 0; f < E && matches < 2; ++f) {
            const HsEvent o = ev[f];
            if (o.kind != kFull || !o.rep || o.table != p.table || o.pos != p.pos) continue;
            const int olen = alt_size(o);
            if (olen < plen) continue;
            const int shift = p.kind == kLeft ? olen - plen : 0;
            bool eq = true;
            for (int i = 0; i < plen && eq; ++i) eq = alt_char(o, shift + i) == alt_char(p, i);
            if (eq) { ++matches; target = f; }
        }
        if (plen == 1) {                                            // SNV keys (ref[pos], base) are keys too
            const int c = base_code(alt_char(p, 0));
            if (kCodeBase[c] == alt_char(p, 0) && snv[p.table][p.pos][c] > 0) { ++matches; target = -2 - c; }
        }
        ev[pi].target = matches == 1 ? target : -1;
    }
    __syncthreads();
    for (int pi = tid; pi < E; pi += 256) {
        const HsEvent p = ev[pi];
        if (p.kind != kFull && p.target <= -2) atomicAdd(&snv[p.table][p.pos][-2 - p.target], p.inc);
    }
    __syncthreads();

    // ---- flagging, kept on the chunk's flag range: the chunk itself for the hotspot stage (AlleleSearcherLite.differingRegions,
    // python/AlleleSearcherLite.py:189-205), one position more on either side for the strict rule of the candidate stage
    const int64_t cb = a.flag_lo[chunk], ce = a.flag_hi[chunk], bb = a.bit_base[chunk];
    auto flag = [&](int64_t p0, int64_t p1) {
        p0 = p0 > cb ? p0 : cb;
        p1 = p1 < ce ? p1 : ce;
        for (int64_t p = p0; p < p1; ++p) {
            const int64_t bit = bb + (p - cb);
            atomicOr(&a.bitmap[bit >> 5], 1u << (bit & 31));
        }
    };
    const float snv_threshold = 0.12f, indel_threshold = 0.12f, min_count = 2.0f;
    for (int i = tid; i < kTile * kCodes; i += 256) {
        const int p = i / kCodes, c = i % kCodes;
        if (!a.hybrid) {                                             // :853-863 with min_count_snv = minCount for both tables
            for (int t = 0; t < 2; ++t) {
                const int v = snv[t][p][c], n = tot[t][p];
                if (v > 0 && n > 0 && (float)v / (float)n >= snv_threshold && (float)v >= min_count) flag(lo + p, lo + p + 1);
            }
        } else if (snv[0][p][c] > 0) {                               // :563-595: keys of counts_i only
            const float total = (float)tot[0][p] + (float)tot[1][p];
            const float vi = (float)snv[0][p][c], vp = (float)snv[1][p][c];
            if (total != 0.0f && (vi + vp) / total >= snv_threshold && vi + vp >= min_count) flag(lo + p, lo + p + 1);
        }
    }
    for (int f = tid; f < E; f += 256) {
        const HsEvent k = ev[f];
        if (k.kind != kFull || !k.rep || (a.hybrid && k.table != 0)) continue;
        int v[2] = {0, 0};
        for (int g = 0; g < E; ++g) {
            const HsEvent o = ev[g];
            if (o.pos != k.pos) continue;
            if (o.kind == kFull ? same_key(o, k) : (o.target >= 0 && same_key(ev[o.target], k))) v[o.table] += o.inc;
        }
        const int64_t p = lo + k.pos;
        if (!a.hybrid) {                                             // :864-885
            const int n = tot[k.table][k.pos];
            const int size = k.ref_len > alt_size(k) ? k.ref_len : alt_size(k);
            const float value = (float)v[k.table], min_indel = k.table == 0 ? 2.0f * min_count : min_count;   // :621,624
            if (n > 0 && size <= 100 && value / (float)n >= indel_threshold && value >= min_indel) flag(p, p + k.ref_len + 1);
        } else {                                                     // :596-605
            const float total = (float)tot[0][k.pos] + (float)tot[1][k.pos];
            const float vi = (float)v[0], vp = (float)v[1];
            if (total != 0.0f && (vi + vp) / total >= indel_threshold && vi / 2 + vp >= min_count) flag(p, p + k.ref_len);
        }
    }
}

}  // namespace
}  // namespace hello
