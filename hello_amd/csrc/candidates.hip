// Candidate sites from hotspot positions (include/hello_mi355x.h: hello_candidates_find): the stage between the hotspot detector
// and the scoring engine, for one Illumina BAM or one PacBio BAM, and (hello_candidates_find_hybrid, at the end of this comment)
// for an Illumina and a PacBio BAM together.
//
// Reference semantics: python/PileupDataTools.py:207-244 (positions -> active regions), :129-158 (the read cap), :302-384 (pass 1:
// one strict searcher per active region), python/trainDataTools.py:477-514 (clusterLocations), :1039-1103 (pass 2: one strict
// searcher per cluster, its own differing regions are the sites), :557-640 and :880-977 (alleles of a site, unsupported and long
// ones dropped), c++/src/Read.cpp:4-172 (a read's allele in a region), c++/src/AlleleSearcherLiteFiltered.cpp:495-547 (strict
// runs), :648-666,740-831 (supports and partials).  DESIGN.md "Candidate sites" restates the rules and the defined orders.
//
// Host: the plan of both passes (read lists with the filters, de-duplication and cap of the hotspot stage, window bounds, tiles
// and exact event capacities over [start - 102, stop]), the clustering between the passes, exact record slots (reads x the
// regions they overlap) and the gather of every allele's reads into the flat arrays of a shard.  Device: the differing-position
// kernel of differing.h for both passes (flags kept on [start - 1, stop] so that the strict rule can be applied), then one
// workgroup per pass-2 cluster for the alleles: a wave per read, a lane per region the read overlaps, one CIGAR walk each ->
// (status, read substring, min_q, hash); the workgroup groups the Success records of a region by string (hash, then bytes),
// resolves the reads' partials against the distinct strings and writes, per region, the alleles in the defined order (reference
// allele, then ascending bytes) with their supporting reads in file order.  Everything is integer and ordered by index, so two
// runs give the same bytes.  Records live in global memory (a cluster's few kilobytes stay in L2); nothing is truncated.
//
// PacBio (HELLO_HOTSPOTS_PACBIO): reads are selected on their original alignment, then every (searcher, kept read) pair is
// strictly clipped (python/PileupContainerLite.py:255-468,554-573: left at the fetch interval's start, then right at its end,
// 201 read bases kept outward of either) by clip_plan_kernel / clip_write_kernel into a derived read set per pass, which the
// kernels above consume unmodified through their read lists; every derived read counts in table 1.
//
// Two BAMs (hello_candidates_find_hybrid; python/AlleleSearcherLite.py:100-206,257-268, c++/src/AlleleSearcherLiteFiltered.cpp:
// 668-738, c++/src/Read.cpp:174-323): every searcher holds the Illumina reads and the clipped PacBio reads, selected and capped
// per container; a pass's reads are ONE set, the Illumina input reads followed by that pass's clipped PacBio copies, with a table
// byte per read, so the differing-position kernel is unchanged.  The allele stage runs as two launches of the same stage function
// (allele_stages) with the reassembly between them: hybrid_records_kernel (records, distinct strings, the Illumina alleles of
// every region in byte order), reassemble_kernel (one wave per (cluster, spanning PacBio read): the read's haplotype is matched
// piecewise against the Illumina alleles, a backward reachability pass and a forward pass that takes the smallest allele by bytes,
// no product is enumerated), hybrid_alleles_kernel (a reassigned read's records are aliases of Illumina records; grouping,
// partials, alleles with the PacBio share of every allele's reads).  The coverage gate is an integer reduction per cluster on the
// host.  allele_kernel is the kWhole instantiation of the same function: the single-BAM launches execute what they did.
//
// Resident (HELLO_CANDIDATES_RESIDENT): the host gather is skipped; the result keeps the pass-2 reads and a gather table per
// technology on the device (keep_resident), and hello_candidates_gather has gather_reads_kernel write the featurizer's per-read
// arrays straight into the scoring loop's launch block.
#include <chrono>
#include <memory>
#include <thread>
#include <unordered_set>

#include "differing.h"
#include "stage_host.h"

namespace hello {
namespace {

// What hello_candidates_gather reads: the reads of pass 2 (rs2), per read the orientation and hp of its input read, and per
// technology the gather table (GatherTable::upload).  Everything is owned by `mem`.
struct Resident {
    DevMem mem;
    const uint8_t* bases = nullptr; const uint8_t* quals = nullptr; const int64_t* read_off = nullptr;
    const uint32_t* cigars = nullptr; const int64_t* cigar_off = nullptr; const int64_t* ref_start = nullptr;
    const uint8_t* mapq = nullptr; const int8_t* orientation = nullptr; const uint8_t* hp = nullptr;
    struct Table { const int64_t* source = nullptr; const int64_t* base_off = nullptr; const int64_t* cigar_off = nullptr;
                   const int32_t* site = nullptr; } table[2];
};

}  // namespace
}  // namespace hello

struct hello_candidates {
    std::vector<int64_t> start, stop, window_start, ref_off{0}, allele_text_off{0}, read_off{0}, cigar_off{0}, ref_start, read_index;
    std::vector<int64_t> regions1, regions2;         // (start, stop) pairs: the differing regions of pass 1 and of pass 2
    std::vector<uint8_t> ref, allele_text, bases, quals, mapq, hp;
    std::vector<int32_t> alleles_per_site, reads_per_allele;
    std::vector<uint32_t> cigars;
    std::vector<int8_t> orientation;
    double stats[HELLO_CANDIDATES_STATS] = {0};
    std::unique_ptr<hello_candidates> second;        // two BAMs: the read arrays of technology 1 (hello_candidates_array_tech)
    double hybrid_stats[HELLO_CANDIDATES_HYBRID_STATS - HELLO_CANDIDATES_STATS] = {0};
    // HELLO_CANDIDATES_RESIDENT: the pass-2 reads and the gather tables on the device (hello_candidates_gather); nullptr for a
    // result without sites, which holds no device memory
    bool resident = false;
    std::unique_ptr<hello::Resident> on_device;
};

namespace hello {
namespace {

constexpr int kSuccess = 0, kLeftPartial = 1, kRightPartial = 2, kFailed = 3;     // AlignedBaseStatus (Read.h)
constexpr int kMaxAlleleLength = 80;                                              // trainDataTools.createTensors
constexpr int kReach = 102;      // an indel of at most 100 bases planted at p flags up to p + 101: tiles start this far left

struct AlleleArgs {
    const uint8_t* bases;
    const uint8_t* quals;
    const int64_t* read_off;
    const uint32_t* cigars;
    const int64_t* cigar_off;
    const int64_t* ref_start;
    const uint8_t* mapq;
    const int64_t* last_pos;          // per read: last M/D position, -1 without one
    const uint8_t* pflags;            // per read: 1 partial_start, 2 partial_stop (Read.cpp:42-49)
    const int64_t* cl_read_off;       // [clusters + 1] into cl_reads
    const int64_t* cl_reads;          // read of every cluster read x
    const int64_t* cl_reg_off;        // [clusters + 1] regions g of a cluster
    const int64_t* reg_start;
    const int64_t* reg_stop;
    const int64_t* rd_rec_off;        // [cluster reads + 1] first record slot of cluster read x; its slots are consecutive regions
    const int64_t* slot_g;            // region of slot s
    const int64_t* slot_x;            // cluster read of slot s
    const int64_t* reg_list_off;      // [regions + 1] into reg_list: the slots of a region, ascending cluster read
    const int64_t* reg_list;
    const uint8_t* ref;               // the chromosome
    int64_t ref_len;
    // records
    int32_t* status;
    int32_t* q0;                      // allele = bases[read_off[r] + q0, + len)
    int32_t* len;
    int32_t* minq;
    uint64_t* hash;
    int32_t* pass;                    // Success with mapq and min_q at their thresholds
    int64_t* first;                   // passing records: the first slot of the region with the same string; else -1
    int64_t* target;                  // the read's chosen partial: the one matching distinct string's slot; else -1
    // output, per region at reg_list_off[g]
    int32_t* n_alleles;               // [regions]
    int64_t* al_rep;                  // slot holding the allele's string
    int32_t* al_count;                // supporting reads
    int64_t* sup;                     // supporting reads (input read index), allele after allele
    int q_threshold, mapq_threshold;
    // two BAMs (hello_candidates_find_hybrid) only
    const uint8_t* tech;              // per read: 0 Illumina, 1 PacBio
    int64_t* alias;                   // records of a reassigned read: the Illumina slot holding its new string; else -1
    uint8_t* reassigned;              // per cluster read
    int64_t* site_al;                 // per region at reg_list_off[g]: the slots of the distinct passing Illumina strings
    int32_t* n_site_al;               //   without N, ascending bytes; their number (> 0: an Illumina site)
    int32_t* al_count1;               // supporting PacBio reads: the last al_count1 of an allele's al_count
};

__device__ void walk_read(const AlleleArgs& a, int64_t r, int64_t s, int64_t e, int64_t slot) {
    // Read::get_aligned_bases(s, e) (Read.cpp:79-137) over the map of Read::_get_read_mapping (:4-77), without building the map
    const int64_t rs = a.ref_start[r], last = a.last_pos[r];
    int status = kFailed, len = 0, minq = 10000;
    int64_t q0 = -1, q1 = -1;
    uint64_t h = 1469598103934665603ull;
    if (last >= 0 && s <= last && rs < e) {                                       // :88
        bool has_s = false, has_sm1 = false, has_em1 = false, has_e = false, emp_s = false, emp_em1 = false, del = false;
        auto mark = [&](int64_t p0, int64_t p1, bool empty) {                     // positions [p0, p1) hold an entry
            if (p0 <= s && s < p1) { has_s = true; emp_s = empty; }
            if (p0 <= s - 1 && s - 1 < p1) has_sm1 = true;
            if (p0 <= e - 1 && e - 1 < p1) { has_em1 = true; emp_em1 = empty; }
            if (p0 <= e && e < p1) has_e = true;
        };
        auto take = [&](int64_t b0, int64_t b1) { if (q0 < 0) q0 = b0; q1 = b1; };
        const int64_t c0 = a.cigar_off[r], n_ops = a.cigar_off[r + 1] - c0;
        int64_t rf = rs, rd = 0;
        for (int64_t ci = 0; ci < n_ops && rf <= e + 1; ++ci) {                   // an entry at e needs rf - 1 <= e
            const unsigned c = a.cigars[c0 + ci];
            const int op = c & 15u;
            const int64_t n = c >> 4;
            if (op == 0 || op == 7 || op == 8) {
                mark(rf, rf + n, false);
                const int64_t lo = rf > s ? rf : s, hi = rf + n < e ? rf + n : e;
                if (lo < hi) take(rd + lo - rf, rd + hi - rf);
                rf += n; rd += n;
            } else if (op == 2) {
                mark(rf, rf + n, true);
                if ((rf > s ? rf : s) < (rf + n < e ? rf + n : e)) del = true;
                rf += n;
            } else if (op == 3) {
                rf += n;
            } else if (op == 1) {                                                 // joins (or creates) the entry at rf - 1
                mark(rf - 1, rf, false);
                if (s <= rf - 1 && rf - 1 < e) take(rd, rd + n);
                rd += n;
            } else if (op == 4) {
                rd += n;
            }
        }
        const int pf = a.pflags[r];
        if (!has_s) status = kLeftPartial;                                        // :94-104
        else if (!has_sm1) status = (pf & 1) ? kLeftPartial : kSuccess;
        else if (!has_em1) status = kRightPartial;
        else if (!has_e) status = (pf & 2) ? kRightPartial : kSuccess;
        else status = kSuccess;
        if ((has_s && emp_s) || (has_em1 && emp_em1)) status = kFailed;          // :107-117
        if (q0 < 0) q0 = q1 = 0;
        len = (int)(q1 - q0);
        const int64_t off = a.read_off[r] + q0;
        int m = del ? 60 : 10000;
        for (int i = 0; i < len; ++i) {
            const int q = a.quals[off + i];
            m = q < m ? q : m;
            h = (h ^ a.bases[off + i]) * 1099511628211ull;
        }
        minq = m;
    }
    a.status[slot] = status;
    a.q0[slot] = (int32_t)(q0 < 0 ? 0 : q0);
    a.len[slot] = len;
    a.minq[slot] = minq;
    a.hash[slot] = h;
    a.pass[slot] = (status == kSuccess && a.mapq[r] >= a.mapq_threshold && minq >= a.q_threshold) ? 1 : 0;   // :766
    a.first[slot] = -1;
    a.target[slot] = -1;
}

// The stages of a cluster's workgroup.  kWhole: all of them, the single-BAM kernel.  Two BAMs run them as two launches with
// the reassembly between: kRecords (the records, the distinct strings, and per region the distinct passing Illumina strings in
// byte order) and kAlleles (the distinct strings again, partials and alleles, a reassigned read's records being its aliases).
constexpr int kWhole = 0, kRecords = 1, kAlleles = 2;

template <int kMode>
__device__ __forceinline__ void allele_stages(const AlleleArgs& a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t c = blockIdx.x;
    const int64_t x0 = a.cl_read_off[c], x1 = a.cl_read_off[c + 1];
    const int64_t g0 = a.cl_reg_off[c], g1 = a.cl_reg_off[c + 1];
    const int64_t s0 = a.rd_rec_off[x0], s1 = a.rd_rec_off[x1];
    auto own_text = [&](int64_t slot) { return a.bases + a.read_off[a.cl_reads[a.slot_x[slot]]] + a.q0[slot]; };
    // the record a slot stands for: itself, or (kAlleles) the Illumina record a reassigned read was given there
    auto src = [&](int64_t slot) -> int64_t {
        if constexpr (kMode == kAlleles) { if (a.reassigned[a.slot_x[slot]] && a.alias[slot] >= 0) return a.alias[slot]; }
        return slot;
    };
    auto passes = [&](int64_t slot) -> bool {
        if constexpr (kMode == kAlleles) {
            const int64_t x = a.slot_x[slot];
            if (a.reassigned[x])                                     // the new records carry min_q 60 (Read.cpp:280)
                return a.alias[slot] >= 0 && a.mapq[a.cl_reads[x]] >= a.mapq_threshold && 60 >= a.q_threshold;
        }
        return a.pass[slot] != 0;
    };
    auto text = [&](int64_t slot) { return own_text(src(slot)); };
    auto length = [&](int64_t slot) { return a.len[src(slot)]; };

    // ---- records: Read::extract_alleles (Read.cpp:139-172), a wave per read, a lane per region the read overlaps
    if constexpr (kMode != kAlleles) {
        for (int64_t x = x0 + wave; x < x1; x += 4) {
            const int64_t r = a.cl_reads[x];
            for (int64_t slot = a.rd_rec_off[x] + lane; slot < a.rd_rec_off[x + 1]; slot += 64) {
                const int64_t g = a.slot_g[slot];
                walk_read(a, r, a.reg_start[g], a.reg_stop[g], slot);
            }
        }
        __syncthreads();
    }

    // ---- the distinct supported strings of every region (AlleleSearcherLiteFiltered.cpp:764-775): hash, then bytes
    for (int64_t slot = s0 + tid; slot < s1; slot += 256) {
        if (!passes(slot)) {
            if constexpr (kMode == kAlleles) a.first[slot] = -1;     // the records stage's answer for a read since reassigned
            continue;
        }
        const int64_t g = a.slot_g[slot];
        const int n = length(slot);
        const uint64_t h = a.hash[src(slot)];
        const uint8_t* mine = text(slot);
        int64_t found = slot;
        for (int64_t i = a.reg_list_off[g]; i < a.reg_list_off[g + 1]; ++i) {
            const int64_t o = a.reg_list[i];
            if (o >= slot) break;
            if (!passes(o) || a.hash[src(o)] != h || length(o) != n) continue;
            const uint8_t* other = text(o);
            bool eq = true;
            for (int k = 0; k < n && eq; ++k) eq = other[k] == mine[k];
            if (eq) { found = o; break; }
        }
        a.first[slot] = found;
    }
    __syncthreads();
    auto less = [&](int64_t x, int64_t y) {                          // bytes of x < bytes of y
        const uint8_t* tx = text(x);
        const uint8_t* ty = text(y);
        const int nx = length(x), ny = length(y), n = nx < ny ? nx : ny;
        for (int k = 0; k < n; ++k)
            if (tx[k] != ty[k]) return tx[k] < ty[k];
        return nx < ny;
    };
    auto has_n = [&](int64_t o) {
        const uint8_t* t = text(o);
        for (int k = 0; k < length(o); ++k)
            if (t[k] == 'N') return true;
        return false;
    };
    if constexpr (kMode == kRecords) {
        // ---- the Illumina alleles of every region (get_alleles_from_reads over the Illumina reads, :698-708), ascending bytes.
        // Illumina reads come first in a cluster, so the first holder of a string an Illumina read spells is an Illumina record.
        for (int64_t g = g0 + tid; g < g1; g += 256) {
            const int64_t l0 = a.reg_list_off[g], l1 = a.reg_list_off[g + 1];
            int n_out = 0;
            int64_t prev = -1;
            for (;;) {
                int64_t best = -1;
                for (int64_t i = l0; i < l1; ++i) {
                    const int64_t o = a.reg_list[i];
                    if (a.first[o] != o || a.tech[a.cl_reads[a.slot_x[o]]] != 0) continue;
                    if (prev >= 0 && !less(prev, o)) continue;
                    if (best >= 0 && !less(o, best)) continue;
                    if (!has_n(o)) best = o;
                }
                if (best < 0) break;
                a.site_al[l0 + n_out++] = best;
                prev = best;
            }
            a.n_site_al[g] = n_out;
        }
        return;
    }

    // ---- partials (:812-831): a read's last left partial, else its last right partial, against the distinct strings of its region
    for (int64_t x = x0 + tid; x < x1; x += 256) {
        int64_t chosen = -1;
        for (int64_t slot = a.rd_rec_off[x + 1] - 1; slot >= a.rd_rec_off[x]; --slot)
            if (a.status[slot] == kLeftPartial) { chosen = slot; break; }
        if (chosen < 0)
            for (int64_t slot = a.rd_rec_off[x + 1] - 1; slot >= a.rd_rec_off[x]; --slot)
                if (a.status[slot] == kRightPartial) { chosen = slot; break; }
        if (chosen < 0) continue;
        const bool left = a.status[chosen] == kLeftPartial;
        const int64_t g = a.slot_g[chosen];
        const int n = a.len[chosen];
        const uint8_t* mine = own_text(chosen);                      // a partial stays as extracted
        int matches = 0;
        int64_t hit = -1;
        for (int64_t i = a.reg_list_off[g]; i < a.reg_list_off[g + 1] && matches < 2; ++i) {
            const int64_t o = a.reg_list[i];
            if (a.first[o] != o || length(o) < n) continue;
            const uint8_t* other = text(o) + (left ? length(o) - n : 0);
            bool eq = true;
            for (int k = 0; k < n && eq; ++k) eq = other[k] == mine[k];
            if (eq) { ++matches; hit = o; }
        }
        if (matches == 1) a.target[chosen] = hit;
    }
    __syncthreads();

    // ---- per region: the reference allele if supported, then the supported strings without N in ascending byte order, none
    // longer than kMaxAlleleLength; every allele's reads in ascending index (trainDataTools.py:612-635,924-946)
    for (int64_t g = g0 + tid; g < g1; g += 256) {
        const int64_t l0 = a.reg_list_off[g], l1 = a.reg_list_off[g + 1];
        const int64_t s = a.reg_start[g], e = a.reg_stop[g];
        int n_out = 0;
        int64_t n_sup = 0;
        auto emit = [&](int64_t rep) {
            int count = 0, count1 = 0;
            for (int64_t i = l0; i < l1; ++i) {
                const int64_t o = a.reg_list[i];
                if ((passes(o) && a.first[o] == rep) || a.target[o] == rep) {
                    a.sup[l0 + n_sup++] = a.cl_reads[a.slot_x[o]];
                    ++count;
                    if constexpr (kMode == kAlleles) count1 += a.tech[a.cl_reads[a.slot_x[o]]];
                }
            }
            a.al_rep[l0 + n_out] = rep;
            a.al_count[l0 + n_out] = count;
            if constexpr (kMode == kAlleles) a.al_count1[l0 + n_out] = count1;
            ++n_out;
        };
        auto is_ref = [&](int64_t o) {
            if (length(o) != e - s || e > a.ref_len) return false;
            const uint8_t* t = text(o);
            for (int64_t k = 0; k < e - s; ++k)
                if (t[k] != a.ref[s + k]) return false;
            return true;
        };
        int64_t ref_rep = -1;
        for (int64_t i = l0; i < l1 && ref_rep < 0; ++i) {
            const int64_t o = a.reg_list[i];
            if (a.first[o] == o && is_ref(o)) ref_rep = o;
        }
        if (ref_rep >= 0 && e - s <= kMaxAlleleLength) emit(ref_rep);
        int64_t prev = -1;
        for (;;) {                                                    // the smallest string above the previous one
            int64_t best = -1;
            for (int64_t i = l0; i < l1; ++i) {
                const int64_t o = a.reg_list[i];
                if (a.first[o] != o || o == ref_rep || length(o) > kMaxAlleleLength) continue;
                if (prev >= 0 && !less(prev, o)) continue;
                if (best >= 0 && !less(o, best)) continue;
                if (!has_n(o)) best = o;
            }
            if (best < 0) break;
            emit(best);
            prev = best;
        }
        a.n_alleles[g] = n_out;
    }
}

__global__ __launch_bounds__(256) void allele_kernel(AlleleArgs a) { allele_stages<kWhole>(a); }
__global__ __launch_bounds__(256) void hybrid_records_kernel(AlleleArgs a) { allele_stages<kRecords>(a); }
__global__ __launch_bounds__(256) void hybrid_alleles_kernel(AlleleArgs a) { allele_stages<kAlleles>(a); }

// ---- reassembly (AlleleSearcherLiteFiltered.cpp:695-738, Read.cpp:174-323): a PacBio read that spans [start, stop) = [first
// region - 6, last region + 6) and whose haplotype there -- the reference with its Success records in place -- is spelled by one
// Illumina allele per Illumina site takes those alleles as its records.  The reference enumerates the product of the sites'
// alleles; here one wave per (cluster, eligible read) matches the haplotype piecewise: reference segment, site allele, reference
// segment ...  A state is (site, offset into the haplotype at which the site's allele begins).  A backward pass over the sites
// marks the states from which the end can be reached, one bit per offset; a forward pass then takes at every site the
// smallest allele by bytes that leads to a marked state, which is the choice with the lexicographically smallest index tuple
// (DESIGN.md "Two BAMs").  The wave owns its haplotype bytes and its bits: every loop is wave-uniform, the lanes compare 64
// bytes per step, lane 0 writes.  The host counted both scratch areas exactly from the records.
struct ReassemblyArgs {
    AlleleArgs a;
    const int64_t* pair_x;            // the cluster read of every (cluster, eligible PacBio read) pair
    const int64_t* pair_c;            // its cluster
    const int64_t* hap_off;           // [pairs + 1] into hap: the haplotype's bytes
    const int64_t* bit_off;           // [pairs + 1] into bits: (regions + 1) rows of (haplotype length + 1) bits, zeroed
    uint8_t* hap;
    unsigned* bits;
    int32_t* result;                  // per pair: 0 unchanged, 1 reassigned, 2 reassigned and several choices spell it, < 0 internal
    int64_t n_pairs;
};

__device__ __forceinline__ bool wave_equal(const uint8_t* x, const uint8_t* y, int64_t n, int lane) {
    for (int64_t i = 0; i < n; i += 64) {
        const bool differ = i + lane < n && x[i + lane] != y[i + lane];
        if (__ballot(differ)) return false;
    }
    return true;
}

__global__ __launch_bounds__(64) void reassemble_kernel(ReassemblyArgs q) {
    const AlleleArgs& a = q.a;
    const int lane = threadIdx.x;
    const int64_t pair = blockIdx.x;
    if (pair >= q.n_pairs) return;
    const int64_t x = q.pair_x[pair], c = q.pair_c[pair];
    const int64_t g0 = a.cl_reg_off[c], g1 = a.cl_reg_off[c + 1], ng = g1 - g0;
    const int64_t slot0 = a.rd_rec_off[x];                           // an eligible read has a record in every region, in order
    const int64_t start = a.reg_start[g0] - 6, stop = a.reg_stop[g1 - 1] + 6;
    uint8_t* hap = q.hap + q.hap_off[pair];
    const int64_t cap = q.hap_off[pair + 1] - q.hap_off[pair];
    auto own_text = [&](int64_t slot) { return a.bases + a.read_off[a.cl_reads[a.slot_x[slot]]] + a.q0[slot]; };
    auto fail = [&](int code) { if (lane == 0) q.result[pair] = code; };

    // ---- Read::get_haplotype_string (Read.cpp:174-203)
    int64_t H = 0;
    bool fits = true;
    auto append = [&](const uint8_t* from, int64_t n) {
        if (H + n > cap) { fits = false; return; }
        for (int64_t i = lane; i < n; i += 64) hap[H + i] = from[i];
        H += n;
    };
    int64_t cur = start;
    for (int64_t g = g0; g < g1 && fits; ++g) {
        const int64_t slot = slot0 + (g - g0);
        append(a.ref + cur, a.reg_start[g] - cur);
        if (a.status[slot] == kSuccess) append(own_text(slot), a.len[slot]);
        else append(a.ref + a.reg_start[g], a.reg_stop[g] - a.reg_start[g]);
        cur = a.reg_stop[g];
    }
    if (fits) append(a.ref + cur, stop - cur);
    if (!fits || H != cap) { fail(-1); return; }
    __syncthreads();

    const int64_t W = (H + 1 + 31) / 32;                               // words of a row
    unsigned* bits = q.bits + q.bit_off[pair];
    if ((ng + 1) * W != q.bit_off[pair + 1] - q.bit_off[pair]) { fail(-2); return; }
    auto row = [&](int64_t k) { return bits + k * W; };
    auto marked = [&](int64_t k, int64_t o) { return (row(k)[o >> 5] >> (o & 31)) & 1u; };

    // ---- backward: the states that reach the end.  Row g - g0 belongs to the site of region g, row ng to the end (offset H).
    if (lane == 0) row(ng)[H >> 5] |= 1u << (H & 31);
    __syncthreads();
    int64_t next_row = ng, next_start = stop;
    for (int64_t g = g1 - 1; g >= g0; --g) {
        const int n_al = a.n_site_al[g];
        if (n_al == 0) continue;                                     // no Illumina site: reference, part of a segment
        const int64_t seg_lo = a.reg_stop[g], seg_n = next_start - seg_lo, l0 = a.reg_list_off[g];
        for (int64_t w = 0; w < W; ++w) {
            unsigned word = row(next_row)[w];
            while (word) {
                const int b = __ffs(word) - 1;
                word &= word - 1;
                const int64_t p = w * 32 + b - seg_n;                // where the segment behind the allele begins
                if (p < 0 || !wave_equal(hap + p, a.ref + seg_lo, seg_n, lane)) continue;
                for (int i = 0; i < n_al; ++i) {
                    const int64_t al = a.site_al[l0 + i];
                    const int64_t n = a.len[al], o = p - n;
                    if (o < 0 || !wave_equal(hap + o, own_text(al), n, lane)) continue;
                    if (lane == 0) row(g - g0)[o >> 5] |= 1u << (o & 31);
                }
            }
        }
        __syncthreads();
        next_row = g - g0;
        next_start = a.reg_start[g];
    }
    if (next_row == ng) { fail(0); return; }                         // no Illumina site: nothing matches (Read.cpp:248-258)

    // ---- forward: the smallest allele by bytes that leads to a marked state, site after site
    int64_t o = next_start - start;                                  // the first site's allele begins behind the first segment
    if (o > H || !wave_equal(hap, a.ref + start, o, lane) || !marked(next_row, o)) { fail(0); return; }
    bool tie = false;
    for (int64_t g = g0 + next_row; g < g1; ++g) {
        const int n_al = a.n_site_al[g];
        if (n_al == 0) continue;
        int64_t after_row = ng, after_start = stop;
        for (int64_t k = g + 1; k < g1; ++k)
            if (a.n_site_al[k] > 0) { after_row = k - g0; after_start = a.reg_start[k]; break; }
        const int64_t seg_lo = a.reg_stop[g], seg_n = after_start - seg_lo, l0 = a.reg_list_off[g];
        int64_t chosen = -1, advance = 0;
        int viable = 0;
        for (int i = 0; i < n_al; ++i) {
            const int64_t al = a.site_al[l0 + i];
            const int64_t n = a.len[al];
            if (o + n + seg_n > H) continue;
            if (!wave_equal(hap + o, own_text(al), n, lane) || !wave_equal(hap + o + n, a.ref + seg_lo, seg_n, lane)) continue;
            if (!marked(after_row, o + n + seg_n)) continue;
            if (viable++ == 0) { chosen = al; advance = n + seg_n; }
        }
        if (chosen < 0) { fail(-3); return; }                        // cannot happen: (g, o) is marked
        tie = tie || viable > 1;
        if (lane == 0) a.alias[slot0 + (g - g0)] = chosen;
        o += advance;
    }
    if (lane == 0) {
        a.reassigned[x] = 1;
        q.result[pair] = tie ? 2 : 1;
    }
}

struct Job {                       // one searcher: an active region (pass 1) or a cluster (pass 2)
    int64_t start, stop;           // the searcher's region
    int64_t fetch_lo, fetch_hi;    // the reads fetched for it
    std::vector<int64_t> reads;    // kept reads, file order
    std::vector<std::pair<int64_t, int64_t>> regions;   // strict differing regions
    bool run = false, capped = false;
};

struct JobStats { int64_t empty = 0, bounds = 0, capped = 0, counted = 0, tiles = 0, events = 0, clipped = 0; float ms = 0, clip_ms = 0; };

// The reads every stage after the selection sees: the input reads themselves, or the clipped copies of one pass (PacBio).
// The view is the set's host arrays (`flags` only on input reads), the layout what strict_walk found in them.
struct ReadSet : ReadsView, ReadLayout {
    const int64_t* origin = nullptr;          // the input read of every read; nullptr: these are the input reads
    // on the device
    DeviceReads d;
    const int64_t* d_ref_end = nullptr; const uint8_t* d_table = nullptr;
    DevMem mem;
    // storage of a derived set
    std::vector<uint8_t> v_bases, v_quals, v_mapq;
    std::vector<int64_t> v_read_off, v_cigar_off, v_ref_start, v_ref_end, v_origin;
    std::vector<uint32_t> v_cigars;
    int64_t input(int64_t r) const { return origin ? origin[r] : r; }
};

// ---- strict clipping (python/PileupContainerLite.py: strictClipFn :255-363, strictClipRead :366-468, __get_reads :554-573)
//
// A clipped read is a slice [q_lo, q_hi) of the read's bases and the operations [a, b] of its CIGAR with new first and last
// operations (a new length; an outermost kept I becomes S).  The reference rejoins the halves of a clip with equal centre
// operations merged: the two halves of the split operation, or, when the clip position is an operation's last base and the next
// operation is of the same kind (20M 20M), those two -- `fuse_l` / `fuse_r` name the first of such a pair, written as one.
constexpr int kClipFlank = 200;                                                   // caller_calling.py:795-843 (clipFlank)

struct ClipRec {
    int64_t a, b;             // first and last kept operation of the read
    int64_t q_lo, q_hi;       // kept read bases
    int64_t ref_start, ref_end;
    int64_t fuse_l, fuse_r;   // operations f and f + 1 are written as one (the left / the right clip's centre); -1: none
    uint32_t first, last;     // their CIGAR words (equal when a == b)
    int32_t clipped;          // 1 the left clip applied, 2 the right clip applied
};

struct ClipArgs {
    const uint8_t* bases; const uint8_t* quals; const int64_t* read_off; const uint32_t* cigars; const int64_t* cigar_off;
    const int64_t* ref_start; const int64_t* ref_end;
    const int64_t* pair_read;         // the input read of every (searcher, kept read) pair
    const int64_t* pair_lo;           // the searcher's fetch interval: clipped left at lo, then right at hi
    const int64_t* pair_hi;
    int64_t n_pairs;
    int flank;
    ClipRec* rec;
    // the second launch
    const int64_t* out_read_off;      // [pairs + 1], the exclusive scans of the first launch's counts
    const int64_t* out_cigar_off;
    uint8_t* out_bases; uint8_t* out_quals; uint32_t* out_cigars;
};

__device__ __forceinline__ bool dev_query_op(int op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
__device__ __forceinline__ bool dev_ref_op(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// First launch, one wave per pair: the lanes stride the CIGAR 64 operations at a time with a wave prefix sum over reference and
// read consumption until the operations holding both clip positions are known; the walks outward of them (at most flank + 1
// read bases each) are wave-uniform.
__global__ __launch_bounds__(256) void clip_plan_kernel(ClipArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= a.n_pairs) return;                                                // wave-uniform
    const int64_t r = a.pair_read[pair], P = a.pair_lo[pair], P2 = a.pair_hi[pair];
    const int64_t c0 = a.cigar_off[r], n = a.cigar_off[r + 1] - c0;
    const int64_t rs = a.ref_start[r], re = a.ref_end[r];
    const uint32_t* cig = a.cigars + c0;
    const bool want_l = rs <= P && P < re, want_r = rs <= P2 && P2 < re;         // :386, before either clip: P < P2
    int64_t il = -1, rc_l = 0, qp_l = 0, ir = -1, rc_r = 0, qp_r = 0;            // the operation holding P / P2, what precedes it
    int64_t ref_run = rs, q_run = 0;
    for (int64_t base = 0; base < n && ((want_l && il < 0) || (want_r && ir < 0)); base += 64) {
        const int64_t idx = base + lane;
        const uint32_t c = idx < n ? cig[idx] : 0u;
        const int op = c & 15u;
        const int64_t len = c >> 4;
        const int64_t dr = dev_ref_op(op) ? len : 0, dq = dev_query_op(op) ? len : 0;
        int64_t sr = dr, sq = dq;
        for (int d = 1; d < 64; d <<= 1) {                                        // inclusive wave scan
            const int64_t ur = __shfl_up(sr, d), uq = __shfl_up(sq, d);
            if (lane >= d) { sr += ur; sq += uq; }
        }
        const int64_t before = ref_run + sr - dr, after = ref_run + sr, q_before = q_run + sq - dq;
        if (want_l && il < 0) {
            const unsigned long long hit = __ballot(idx < n && before <= P && P < after);
            if (hit) {
                const int src = __ffsll(hit) - 1;
                il = base + src; rc_l = __shfl(before, src); qp_l = __shfl(q_before, src);
            }
        }
        if (want_r && ir < 0) {
            const unsigned long long hit = __ballot(idx < n && before <= P2 && P2 < after);
            if (hit) {
                const int src = __ffsll(hit) - 1;
                ir = base + src; rc_r = __shfl(before, src); qp_r = __shfl(q_before, src);
            }
        }
        ref_run += __shfl(sr, 63);
        q_run += __shfl(sq, 63);
    }
    ClipRec o;
    o.a = 0; o.b = n - 1; o.q_lo = 0; o.q_hi = a.read_off[r + 1] - a.read_off[r]; o.ref_start = rs; o.ref_end = re;
    o.first = cig[0]; o.last = cig[n - 1]; o.clipped = 0; o.fuse_l = -1; o.fuse_r = -1;
    int64_t len_a = o.first >> 4;                                                  // current length of operation a
    if (il >= 0) {                                                                 // left clip at P (:424-433)
        const int op_i = cig[il] & 15u;
        const int64_t len_i = cig[il] >> 4, k = P - rc_l + 1;                      // the left half takes k of operation il (:405)
        int64_t count = 0, kept_ref = 0, kept_q = 0, keep = 0;
        for (int64_t idx = il; idx >= 0; --idx) {                                  // strictClipFn, leftwards
            const int op = cig[idx] & 15u;
            const int64_t len = idx == il ? k : (int64_t)(cig[idx] >> 4);
            const int64_t qn = dev_query_op(op) ? len : 0;
            o.a = idx;
            if (count <= a.flank && a.flank < count + qn) {                        // :288-301
                keep = a.flank - count + 1;
                kept_q += keep;
                kept_ref += dev_ref_op(op) ? keep : 0;
                break;
            }
            keep = len;
            kept_q += qn;
            kept_ref += dev_ref_op(op) ? len : 0;
            count += qn;
        }
        int op_a = cig[o.a] & 15u;
        if (op_a == 1) op_a = 4;                                                   // a kept leading I becomes S (:315-319)
        len_a = o.a == il ? keep + (len_i - k) : keep;                             // the halves of operation il are rejoined (:457)
        o.first = (uint32_t)(len_a << 4) | (uint32_t)op_a;
        o.ref_start = P + 1 - kept_ref;
        o.q_lo = qp_l + (dev_query_op(op_i) ? k : 0) - kept_q;
        o.clipped |= 1;
        if (o.a == o.b) o.last = o.first;
        if (k == len_i && il + 1 < n && (int)(cig[il + 1] & 15u) == op_i) o.fuse_l = il;      // equal centre operations (:457)
    }
    if (ir >= 0) {                                                                 // right clip at P2 (:434-449), on that result
        const int op_j = cig[ir] & 15u;
        const int64_t len_j = cig[ir] >> 4, part = P2 - rc_r + 1, rest = len_j - part;   // operation ir ends where it did
        int64_t count = 0, kept_ref = 0, kept_q = 0, keep = 0, b = -1;
        for (int64_t idx = rest > 0 ? ir : ir + 1; idx < n; ++idx) {               // strictClipFn, rightwards
            const int op = cig[idx] & 15u;
            const int64_t len = idx == ir ? rest : (int64_t)(cig[idx] >> 4);
            const int64_t qn = dev_query_op(op) ? len : 0;
            b = idx;
            if (count <= a.flank && a.flank < count + qn) {
                keep = a.flank - count + 1;
                kept_q += keep;
                kept_ref += dev_ref_op(op) ? keep : 0;
                break;
            }
            keep = len;
            kept_q += qn;
            kept_ref += dev_ref_op(op) ? len : 0;
            count += qn;
        }
        if (b >= 0) {                                                              // an empty right half changes nothing (:434)
            int op_b = cig[b] & 15u;
            if (op_b == 1) op_b = 4;                                               // a kept trailing I becomes S (:321-324)
            const int64_t len_b = b == ir ? (ir == o.a ? len_a : len_j) - rest + keep : keep;
            o.b = b;
            o.last = (uint32_t)(len_b << 4) | (uint32_t)op_b;
            if (o.a == o.b) o.first = o.last;
            o.ref_end = P2 + 1 + kept_ref;
            o.q_hi = qp_r + (dev_query_op(op_j) ? part : 0) + kept_q;
            o.clipped |= 2;
            if (rest == 0 && (int)(cig[ir + 1] & 15u) == op_j) o.fuse_r = ir;
        }
    }
    if (lane == 0) a.rec[pair] = o;
}

// Second launch, one wave per pair: the lanes copy the kept operations (first and last replaced) and the kept bases and
// qualities to the pair's place in the derived set.
__global__ __launch_bounds__(256) void clip_write_kernel(ClipArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= a.n_pairs) return;
    const ClipRec o = a.rec[pair];
    const int64_t r = a.pair_read[pair];
    const uint32_t* cig = a.cigars + a.cigar_off[r];
    uint32_t* out = a.out_cigars + a.out_cigar_off[pair];
    auto word = [&](int64_t x) { return x == o.a ? o.first : (x == o.b ? o.last : cig[x]); };   // operation x as clipped
    for (int64_t x = o.a + lane; x <= o.b; x += 64) {
        if ((o.fuse_l >= 0 && x == o.fuse_l + 1) || (o.fuse_r >= 0 && x == o.fuse_r + 1)) continue;     // written with x - 1
        uint32_t w = word(x);
        int64_t last = x;                                                          // the run x .. last is one operation
        if (o.fuse_l >= 0 && last == o.fuse_l) ++last;
        if (o.fuse_r >= 0 && last == o.fuse_r) ++last;
        for (int64_t y = x + 1; y <= last; ++y) w += word(y) & ~15u;
        out[x - o.a - (o.fuse_l >= 0 && x > o.fuse_l ? 1 : 0) - (o.fuse_r >= 0 && x > o.fuse_r ? 1 : 0)] = w;
    }
    const int64_t src = a.read_off[r] + o.q_lo, dst = a.out_read_off[pair], n_bases = a.out_read_off[pair + 1] - dst;
    for (int64_t i = lane; i < n_bases; i += 64) {
        a.out_bases[dst + i] = a.bases[src + i];
        a.out_quals[dst + i] = a.quals[src + i];
    }
}

// The kept reads of every job (PileupContainerLite.__get_reads :526-570 under the cap of ReadSampler.__call__,
// PileupDataTools.py:139-146), on the original alignments.
void select_reads(std::vector<Job>& jobs, const ReadsView& in, int64_t max_span, bool pacbio, JobStats& st) {
    std::unordered_set<std::pair<uint64_t, int>, PairHash> seen;
    for (Job& job : jobs) {
        const int64_t span = job.fetch_hi - job.fetch_lo;
        const double cap = pacbio ? (span > 100 ? 100.0 / 100.0 * (double)span : 100.0)
                                  : (span > 30 ? 1000.0 / 30.0 * (double)span : 1000.0);
        seen.clear();
        const int64_t* begin = in.ref_start;
        const int64_t* it = std::lower_bound(begin, begin + in.n, job.fetch_lo - max_span);
        for (int64_t r = it - begin; r < in.n && in.ref_start[r] < job.fetch_hi; ++r) {
            if (in.ref_end[r] <= job.fetch_lo || !usable(in.flags[r], in.mapq[r])) continue;
            if (!seen.insert({in.name_hash[r], (in.flags[r] & 16) ? 1 : 0}).second) continue;
            if (!((double)job.reads.size() < cap)) { job.capped = true; continue; }
            job.reads.push_back(r);
        }
        if (job.reads.empty()) ++st.empty;
    }
}

// PacBio: the clipped copy of every (job, kept read) pair as the reads of `out`; job.reads become indices into it.
void clip_reads(std::vector<Job>& jobs, const ReadsView& in, const ReadSet& input, ReadSet& out, JobStats& st) {
    std::vector<int64_t> pair_read, pair_lo, pair_hi;
    for (Job& job : jobs)
        for (int64_t& r : job.reads) {
            pair_read.push_back(r);
            pair_lo.push_back(job.fetch_lo);
            pair_hi.push_back(job.fetch_hi);
            r = (int64_t)pair_read.size() - 1;
        }
    const int64_t n = (int64_t)pair_read.size();
    out.n = n;
    out.v_origin = pair_read;
    out.v_read_off.assign((size_t)n + 1, 0);
    out.v_cigar_off.assign((size_t)n + 1, 0);
    out.v_ref_start.resize((size_t)n);
    out.v_ref_end.resize((size_t)n);
    out.v_mapq.resize((size_t)n);
    if (n > 0) {
        DevMem m;
        ClipArgs c{};
        c.bases = input.d.bases; c.quals = input.d.quals; c.read_off = input.d.read_off; c.cigars = input.d.cigars;
        c.cigar_off = input.d.cigar_off; c.ref_start = input.d.ref_start; c.ref_end = input.d_ref_end;
        c.pair_read = m.put(pair_read.data(), pair_read.size());
        c.pair_lo = m.put(pair_lo.data(), pair_lo.size());
        c.pair_hi = m.put(pair_hi.data(), pair_hi.size());
        c.n_pairs = n;
        c.flank = kClipFlank;
        c.rec = m.zeros<ClipRec>((size_t)n);
        const dim3 grid((unsigned)((n + 3) / 4));
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(clip_plan_kernel, grid, dim3(256), 0, 0, c);
        st.clip_ms = timer.stop();
        std::vector<ClipRec> rec((size_t)n);
        HS_HIP(hipMemcpy(rec.data(), c.rec, rec.size() * sizeof(ClipRec), hipMemcpyDeviceToHost));
        for (int64_t p = 0; p < n; ++p) {                      // the second launch writes within these: checked before it runs
            const ClipRec& o = rec[p];
            const int64_t r = pair_read[p], n_ops = in.cigar_off[r + 1] - in.cigar_off[r], n_bases = in.read_off[r + 1] - in.read_off[r];
            const bool fuse_ok = (o.fuse_l < 0 || (o.fuse_l >= o.a && o.fuse_l < o.b)) && (o.fuse_r < 0 || (o.fuse_r >= o.a && o.fuse_r < o.b)) &&
                                 (o.fuse_l < 0 || o.fuse_l != o.fuse_r);
            if (o.a < 0 || o.b < o.a || o.b >= n_ops || o.q_lo < 0 || o.q_hi < o.q_lo || o.q_hi > n_bases || !fuse_ok)
                raise(HELLO_ERR_ARG, "internal: the clip of read %lld leaves the read", (long long)r);
            out.v_cigar_off[p + 1] = out.v_cigar_off[p] + (o.b - o.a + 1) - (o.fuse_l >= 0 ? 1 : 0) - (o.fuse_r >= 0 ? 1 : 0);
            out.v_read_off[p + 1] = out.v_read_off[p] + (o.q_hi - o.q_lo);
            out.v_ref_start[p] = o.ref_start;
            out.v_ref_end[p] = o.ref_end;
            out.v_mapq[p] = in.mapq[r];
            st.clipped += o.clipped ? 1 : 0;
        }
        const size_t nb = (size_t)out.v_read_off[n], nc = (size_t)out.v_cigar_off[n];
        out.d.read_off = c.out_read_off = out.mem.put(out.v_read_off.data(), out.v_read_off.size());
        out.d.cigar_off = c.out_cigar_off = out.mem.put(out.v_cigar_off.data(), out.v_cigar_off.size());
        out.d.bases = c.out_bases = out.mem.zeros<uint8_t>(nb);
        out.d.quals = c.out_quals = out.mem.zeros<uint8_t>(nb);
        out.d.cigars = c.out_cigars = out.mem.zeros<uint32_t>(nc);
        timer.start();
        hipLaunchKernelGGL(clip_write_kernel, grid, dim3(256), 0, 0, c);
        st.clip_ms += timer.stop();
        out.v_bases.resize(nb);
        out.v_quals.resize(nb);
        out.v_cigars.resize(nc);
        if (nb) HS_HIP(hipMemcpy(out.v_bases.data(), c.out_bases, nb, hipMemcpyDeviceToHost));
        if (nb) HS_HIP(hipMemcpy(out.v_quals.data(), c.out_quals, nb, hipMemcpyDeviceToHost));
        if (nc) HS_HIP(hipMemcpy(out.v_cigars.data(), c.out_cigars, nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
        out.d.ref_start = out.mem.put(out.v_ref_start.data(), out.v_ref_start.size());
        out.d_ref_end = out.mem.put(out.v_ref_end.data(), out.v_ref_end.size());
        const std::vector<uint8_t> table((size_t)n, 1);             // every read counts in the PacBio table, increment 1
        out.d_table = out.mem.put(table.data(), table.size());
    }
    out.bases = out.v_bases.data(); out.quals = out.v_quals.data(); out.read_off = out.v_read_off.data();
    out.cigars = out.v_cigars.data(); out.cigar_off = out.v_cigar_off.data(); out.ref_start = out.v_ref_start.data();
    out.ref_end = out.v_ref_end.data(); out.mapq = out.v_mapq.data(); out.origin = out.v_origin.data();
    strict_walk(out, kStrictRegions, out, out.origin);
}

// The window and differing regions of every job with reads (AlleleSearcherLite.__init__ + determineDifferingRegions(strict = True)).
void differing_regions(std::vector<Job>& jobs, const ReadSet& in, int64_t reference_length, int mapq_threshold, HotspotArgs a,
                       JobStats& st) {
    const std::vector<int64_t>& plant_off = in.plant_off;
    const std::vector<int64_t>& plant = in.plant;
    std::vector<int64_t> flo, fhi, bit_base, creads_off{0}, creads, tile_lo, tile_ev_off{0};
    std::vector<int32_t> tile_chunk, chunk_job;
    int64_t bits = 0;
    a.bases = in.d.bases; a.quals = in.d.quals; a.read_off = in.d.read_off; a.cigars = in.d.cigars; a.cigar_off = in.d.cigar_off;
    a.ref_start = in.d.ref_start; a.ref_end = in.d_ref_end; a.table = in.d_table;
    for (size_t j = 0; j < jobs.size(); ++j) {
        Job& job = jobs[j];
        const bool capped = job.capped;
        if (job.reads.empty()) continue;
        int64_t ws = job.start, we = INT64_MIN;                                      // AlleleSearcherLite.py:135-151
        for (int64_t r : job.reads) { ws = std::min(ws, in.ref_start[r]); we = std::max(we, in.ref_end[r]); }
        ws -= 10;
        if (ws < 0 || we > reference_length) { ++st.bounds; job.reads.clear(); continue; }
        st.capped += capped;                                                         // counted for searchers that run
        job.run = true;
        const int32_t chunk = (int32_t)flo.size();
        chunk_job.push_back((int32_t)j);
        flo.push_back(job.start - 1);                                                // the strict rule looks at start - 1 and at stop
        fhi.push_back(job.stop + 1);
        bit_base.push_back(bits);
        bits += job.stop - job.start + 2;
        int64_t lo0 = INT64_MAX, hi0 = INT64_MIN;
        const size_t first = creads.size();
        for (int64_t r : job.reads)
            if (in.mapq[r] >= mapq_threshold) {
                creads.push_back(r);
                lo0 = std::min(lo0, in.ref_start[r] - 1);
                hi0 = std::max(hi0, in.ref_end[r]);
            }
        creads_off.push_back((int64_t)creads.size());
        lo0 = std::max(lo0, job.start - kReach);
        hi0 = std::min(hi0, job.stop + 1);
        if (creads.size() == first || lo0 >= hi0) continue;
        const int64_t nt = (hi0 - lo0 + kTile - 1) / kTile;
        std::vector<int64_t> capacity(nt, 0);
        for (size_t k = first; k < creads.size(); ++k) {
            const int64_t r = creads[k];
            for (int64_t i = plant_off[r]; i < plant_off[r + 1]; ++i)
                if (plant[i] >= lo0 && plant[i] < lo0 + nt * kTile) ++capacity[(plant[i] - lo0) / kTile];
        }
        for (int64_t t = 0; t < nt; ++t) {
            tile_chunk.push_back(chunk);
            tile_lo.push_back(lo0 + t * kTile);
            tile_ev_off.push_back(tile_ev_off.back() + capacity[t]);
        }
    }
    st.counted = (int64_t)creads.size();
    st.tiles = (int64_t)tile_lo.size();
    st.events = tile_ev_off.back();
    if (tile_lo.empty()) return;
    DevMem m;
    a.chunk_reads = m.put(creads.data(), creads.size());
    a.chunk_reads_off = m.put(creads_off.data(), creads_off.size());
    a.flag_lo = m.put(flo.data(), flo.size());
    a.flag_hi = m.put(fhi.data(), fhi.size());
    a.bit_base = m.put(bit_base.data(), bit_base.size());
    a.tile_chunk = m.put(tile_chunk.data(), tile_chunk.size());
    a.tile_lo = m.put(tile_lo.data(), tile_lo.size());
    a.tile_ev_off = m.put(tile_ev_off.data(), tile_ev_off.size());
    a.events = m.zeros<HsEvent>((size_t)tile_ev_off.back());
    const int64_t words = (bits + 31) / 32;
    a.bitmap = m.zeros<unsigned>((size_t)words);
    {
        KernelTimer timer;
        timer.start();
        hipLaunchKernelGGL(hotspot_kernel, dim3((unsigned)tile_lo.size()), dim3(256), 0, 0, a);
        st.ms = timer.stop();
    }
    std::vector<unsigned> bitsv((size_t)words);
    HS_HIP(hipMemcpy(bitsv.data(), a.bitmap, bitsv.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    auto bit = [&](int64_t i) { return (bitsv[i >> 5] >> (i & 31)) & 1u; };
    for (size_t c = 0; c < chunk_job.size(); ++c) {            // cluster_differing_regions_helper + pushRegions(strict) (:495-547)
        Job& job = jobs[chunk_job[c]];
        const int64_t n = job.stop - job.start + 2;
        for (int64_t i = 0; i < n;) {
            if (!bit(bit_base[c] + i)) { ++i; continue; }
            int64_t k = i;
            while (k + 1 < n && bit(bit_base[c] + k + 1)) ++k;
            const int64_t first = job.start - 1 + i, last = job.start - 1 + k;
            if (!(first < job.start || last + 1 > job.stop)) job.regions.push_back({first, last + 1});
            i = k + 1;
        }
    }
}

// hotspotsReader (PileupDataTools.py:207-244) and candidateReader's fetch (:347-352): the searchers of pass 1
std::vector<Job> active_region_jobs(const int64_t* positions, int64_t n_positions) {
    std::vector<Job> jobs;
    for (int64_t i = 0; i < n_positions;) {
        int64_t k = i;
        while (k + 1 < n_positions && positions[k + 1] - positions[k] <= 30) ++k;
        Job j;
        j.start = positions[i] - 15;
        j.stop = positions[k] + 15;
        j.fetch_lo = std::max<int64_t>(0, j.start - 75);
        j.fetch_hi = j.stop + 75;
        jobs.push_back(std::move(j));
        i = k + 1;
    }
    return jobs;
}

// The differing regions of pass 1 in order, also as the result's regions1.
std::vector<std::pair<int64_t, int64_t>> pass1_locations(const std::vector<Job>& jobs1, hello_candidates& res) {
    std::vector<std::pair<int64_t, int64_t>> locations;
    for (const Job& j : jobs1)
        for (const auto& reg : j.regions) {
            // strict runs lie inside [first - 15, last + 15] and points of different active regions are > 30 apart: the
            // reference's merge_overlaps (:377-378) has nothing to merge
            if (!locations.empty() && reg.first <= locations.back().second) raise(HELLO_ERR_ARG, "internal: differing regions overlap");
            locations.push_back(reg);
        }
    for (const auto& reg : locations) { res.regions1.push_back(reg.first); res.regions1.push_back(reg.second); }
    return locations;
}

// clusterLocations (trainDataTools.py:477-514, MAX_ITEMS_PER_GROUP = 1024, caller_calling.py:859) and the searcher of every
// cluster (:1045-1065): the searchers of pass 2
std::vector<Job> cluster_jobs(const std::vector<std::pair<int64_t, int64_t>>& locations) {
    std::vector<Job> jobs2;
    std::vector<std::pair<int64_t, int64_t>> cluster;
    auto close = [&]() {
        if (cluster.empty()) return;
        Job j;
        j.start = cluster.front().first - 15;
        j.stop = cluster.back().second + 14;
        j.fetch_lo = j.start;
        j.fetch_hi = j.stop;
        jobs2.push_back(std::move(j));
        cluster.clear();
    };
    for (const auto& loc : locations) {
        if (loc.second - loc.first > kMaxAlleleLength && !cluster.empty()) { close(); continue; }   // the location is dropped
        if (cluster.empty()) cluster.push_back(loc);
        else if (loc.first - cluster.back().second < 30 && cluster.size() < 1024) cluster.push_back(loc);
        else { close(); cluster.push_back(loc); }
    }
    close();
    return jobs2;
}

// The allele stage's plan: record slots = reads x the regions they overlap, counted exactly.
struct AllelePlan {
    std::vector<int64_t> cl_read_off{0}, cl_reads, cl_reg_off{0}, cl_job, reg_start, reg_stop, rd_rec_off{0}, slot_g, slot_x;
    std::vector<int64_t> reg_list_off, reg_list;
    int64_t n_slots = 0, n_reg = 0, n_cl = 0;

    void build(const std::vector<Job>& jobs2, const ReadSet& rs2, hello_candidates& res) {
        for (size_t ji = 0; ji < jobs2.size(); ++ji) {
            const Job& j = jobs2[ji];
            if (j.regions.empty()) continue;
            const int64_t gbase = (int64_t)reg_start.size();
            for (const auto& reg : j.regions) {
                reg_start.push_back(reg.first);
                reg_stop.push_back(reg.second);
                res.regions2.push_back(reg.first);
                res.regions2.push_back(reg.second);
            }
            const int64_t ng = (int64_t)j.regions.size();
            for (int64_t r : j.reads) {
                const int64_t x = (int64_t)cl_reads.size();
                cl_reads.push_back(r);
                if (rs2.last_pos[r] >= 0)                              // Read.cpp:88: start <= last_position && reference_start < stop
                    for (int64_t g = 0; g < ng; ++g)
                        if (j.regions[g].first <= rs2.last_pos[r] && rs2.ref_start[r] < j.regions[g].second) {
                            slot_g.push_back(gbase + g);
                            slot_x.push_back(x);
                        }
                rd_rec_off.push_back((int64_t)slot_g.size());
            }
            cl_read_off.push_back((int64_t)cl_reads.size());
            cl_reg_off.push_back((int64_t)reg_start.size());
            cl_job.push_back((int64_t)ji);
        }
        n_slots = (int64_t)slot_g.size();
        n_reg = (int64_t)reg_start.size();
        n_cl = (int64_t)cl_read_off.size() - 1;
        reg_list_off.assign(n_reg + 1, 0);
        reg_list.resize((size_t)n_slots);
        for (int64_t s = 0; s < n_slots; ++s) ++reg_list_off[slot_g[s] + 1];
        for (int64_t g = 0; g < n_reg; ++g) reg_list_off[g + 1] += reg_list_off[g];
        std::vector<int64_t> fill(reg_list_off.begin(), reg_list_off.end() - 1);
        for (int64_t s = 0; s < n_slots; ++s) reg_list[fill[slot_g[s]]++] = s;      // ascending slot = ascending read
    }

    AlleleArgs upload(DevMem& m, const ReadSet& rs2, const uint8_t* d_ref, int64_t reference_length, int q_threshold,
                      int mapq_threshold) const {
        AlleleArgs b{};
        b.bases = rs2.d.bases; b.quals = rs2.d.quals; b.read_off = rs2.d.read_off; b.cigars = rs2.d.cigars;
        b.cigar_off = rs2.d.cigar_off; b.ref_start = rs2.d.ref_start;
        b.mapq = m.put(rs2.mapq, (size_t)rs2.n);
        b.last_pos = m.put(rs2.last_pos.data(), rs2.last_pos.size());
        b.pflags = m.put(rs2.pflags.data(), rs2.pflags.size());
        b.cl_read_off = m.put(cl_read_off.data(), cl_read_off.size());
        b.cl_reads = m.put(cl_reads.data(), cl_reads.size());
        b.cl_reg_off = m.put(cl_reg_off.data(), cl_reg_off.size());
        b.reg_start = m.put(reg_start.data(), reg_start.size());
        b.reg_stop = m.put(reg_stop.data(), reg_stop.size());
        b.rd_rec_off = m.put(rd_rec_off.data(), rd_rec_off.size());
        b.slot_g = m.put(slot_g.data(), slot_g.size());
        b.slot_x = m.put(slot_x.data(), slot_x.size());
        b.reg_list_off = m.put(reg_list_off.data(), reg_list_off.size());
        b.reg_list = m.put(reg_list.data(), reg_list.size());
        b.ref = d_ref;
        b.ref_len = reference_length;
        b.status = m.zeros<int32_t>((size_t)n_slots);
        b.q0 = m.zeros<int32_t>((size_t)n_slots);
        b.len = m.zeros<int32_t>((size_t)n_slots);
        b.minq = m.zeros<int32_t>((size_t)n_slots);
        b.hash = m.zeros<uint64_t>((size_t)n_slots);
        b.pass = m.zeros<int32_t>((size_t)n_slots);
        b.first = m.zeros<int64_t>((size_t)n_slots);
        b.target = m.zeros<int64_t>((size_t)n_slots);
        b.n_alleles = m.zeros<int32_t>((size_t)n_reg);
        b.al_rep = m.zeros<int64_t>((size_t)n_slots);
        b.al_count = m.zeros<int32_t>((size_t)n_slots);
        b.sup = m.zeros<int64_t>((size_t)n_slots);
        b.q_threshold = q_threshold;
        b.mapq_threshold = mapq_threshold;
        return b;
    }
};

template <class T> void fetch(std::vector<T>& to, const T* from) {
    if (!to.empty()) HS_HIP(hipMemcpy(to.data(), from, to.size() * sizeof(T), hipMemcpyDeviceToHost));
}

struct AlleleResult {
    std::vector<int32_t> n_alleles, al_count, al_count1, rec_q0, rec_len;
    std::vector<int64_t> al_rep, sup;
    explicit AlleleResult(const AllelePlan& p)
        : n_alleles((size_t)p.n_reg, 0), al_count((size_t)p.n_slots), rec_q0((size_t)p.n_slots), rec_len((size_t)p.n_slots),
          al_rep((size_t)p.n_slots), sup((size_t)p.n_slots) {}
    void download(const AlleleArgs& b) {
        fetch(n_alleles, b.n_alleles);
        fetch(al_count, b.al_count);
        fetch(al_rep, b.al_rep);
        fetch(sup, b.sup);
        fetch(rec_q0, b.q0);
        fetch(rec_len, b.len);
        if (b.al_count1) { al_count1.resize(al_count.size()); fetch(al_count1, b.al_count1); }
    }
};

// The sites and, per technology, every allele's reads as indices into rs2 (read_index) with their offsets.  With two
// technologies an allele's PacBio reads are the last al_count1 of its supporting reads.  -> sites dropped at the chromosome's ends
int64_t emit_sites(hello_candidates& o, hello_candidates* second, const AllelePlan& p, const AlleleResult& got, const ReadSet& rs2,
                   const uint8_t* reference, int64_t reference_length, int64_t feature_length) {
    int64_t sites_oob = 0;
    auto add = [&](hello_candidates& to, int64_t r) {
        to.read_index.push_back(r);
        to.read_off.push_back(to.read_off.back() + (rs2.read_off[r + 1] - rs2.read_off[r]));
        to.cigar_off.push_back(to.cigar_off.back() + (rs2.cigar_off[r + 1] - rs2.cigar_off[r]));
    };
    for (int64_t g = 0; g < p.n_reg; ++g) {
        if (got.n_alleles[g] == 0) continue;                                         // caller_calling.py:876
        const int64_t s = p.reg_start[g], e = p.reg_stop[g], L = feature_length;
        const int64_t lo = (s + e) / 2 - L / 2;
        const int64_t ws = std::min(lo, s - 1), we = std::max(lo + L, e);            // one anchor base left of the site
        if (ws < 0 || we > reference_length) { ++sites_oob; continue; }
        o.start.push_back(s);
        o.stop.push_back(e);
        o.window_start.push_back(ws);
        o.ref.insert(o.ref.end(), reference + ws, reference + we);
        o.ref_off.push_back((int64_t)o.ref.size());
        o.alleles_per_site.push_back(got.n_alleles[g]);
        int64_t at = p.reg_list_off[g];
        for (int32_t k = 0; k < got.n_alleles[g]; ++k) {
            const int64_t rep = got.al_rep[p.reg_list_off[g] + k];
            const uint8_t* t = rs2.bases + rs2.read_off[p.cl_reads[p.slot_x[rep]]] + got.rec_q0[rep];
            o.allele_text.insert(o.allele_text.end(), t, t + got.rec_len[rep]);
            o.allele_text_off.push_back((int64_t)o.allele_text.size());
            const int32_t n = got.al_count[p.reg_list_off[g] + k];
            const int32_t n1 = second ? got.al_count1[p.reg_list_off[g] + k] : 0;
            o.reads_per_allele.push_back(n - n1);
            for (int32_t i = 0; i < n - n1; ++i) add(o, got.sup[at + i]);
            if (second) {
                second->reads_per_allele.push_back(n1);
                for (int32_t i = n - n1; i < n; ++i) add(*second, got.sup[at + i]);
            }
            at += n;
        }
    }
    return sites_oob;
}

// The gather of every allele's reads into the arrays of a shard (hello_amd/shards.py): read_index names reads of rs2 on entry
// and the input reads of `flags` / `hp` on return.
void gather_reads(hello_candidates& o, const ReadSet& rs2, const uint16_t* flags, const uint8_t* hp) {
    const int64_t R = (int64_t)o.read_index.size();
    o.bases.resize((size_t)o.read_off.back());
    o.quals.resize((size_t)o.read_off.back());
    o.cigars.resize((size_t)o.cigar_off.back());
    o.ref_start.resize((size_t)R);
    o.mapq.resize((size_t)R);
    o.orientation.resize((size_t)R);
    o.hp.resize((size_t)R);
    const int n_threads = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(), R / 4096 + 1}));
    auto copy = [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t r = o.read_index[i];
            std::copy(rs2.bases + rs2.read_off[r], rs2.bases + rs2.read_off[r + 1], o.bases.begin() + o.read_off[i]);
            std::copy(rs2.quals + rs2.read_off[r], rs2.quals + rs2.read_off[r + 1], o.quals.begin() + o.read_off[i]);
            std::copy(rs2.cigars + rs2.cigar_off[r], rs2.cigars + rs2.cigar_off[r + 1], o.cigars.begin() + o.cigar_off[i]);
            o.ref_start[i] = rs2.ref_start[r];
            o.mapq[i] = rs2.mapq[r];
            o.orientation[i] = (flags[rs2.input(r)] & 16) ? -1 : 1;
            o.hp[i] = hp[rs2.input(r)];
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(copy, R * t / n_threads, R * (t + 1) / n_threads);
    copy(0, R / n_threads);
    for (auto& th : pool) th.join();
    for (int64_t& r : o.read_index) r = rs2.input(r);                      // the input read of a clipped read
}

// ---- resident candidates (HELLO_CANDIDATES_RESIDENT)

// The featurizer's reads of one technology (shards.py: PackedShard.featurizer_core): every allele's supporting reads, an
// allele without one gets a dummy read.  source: per output read the index of the supporting read among the technology's
// supporting reads (allele after allele, the numbering of read_off / cigar_off), -1 for a dummy; base_off / cigar_off: the
// exclusive scans of the output reads' base and CIGAR counts (a dummy has none); site: the site of every output read.
struct GatherTable {
    std::vector<int64_t> source, base_off{0}, cigar_off{0};
    std::vector<int32_t> site;

    void build(const int32_t* reads_per_allele, int64_t n_alleles, const int64_t* read_off, const int64_t* cig_off,
               const int32_t* alleles_per_site, int64_t n_sites) {
        int64_t i = 0, al = 0;
        auto allele = [&](int32_t s) {
            const int32_t n = reads_per_allele[al++];
            for (int32_t k = 0; k < std::max(n, 1); ++k) {
                const bool real = k < n;
                source.push_back(real ? i : -1);
                base_off.push_back(base_off.back() + (real ? read_off[i + 1] - read_off[i] : 0));
                cigar_off.push_back(cigar_off.back() + (real ? cig_off[i + 1] - cig_off[i] : 0));
                site.push_back(s);
                i += real;
            }
        };
        if (alleles_per_site)
            for (int64_t s = 0; s < n_sites; ++s)
                for (int32_t k = 0; k < alleles_per_site[s]; ++k) allele((int32_t)s);
        else
            while (al < n_alleles) allele(0);
    }
};

struct GatherArgs {
    const uint8_t* bases; const uint8_t* quals; const int64_t* read_off; const uint32_t* cigars; const int64_t* cigar_off;
    const int64_t* ref_start; const uint8_t* mapq; const int8_t* orientation; const uint8_t* hp;        // the reads of pass 2
    const int64_t* source; const int64_t* t_base_off; const int64_t* t_cigar_off; const int32_t* site;  // the gather table
    uint8_t* out_bases; uint8_t* out_quals; int64_t* out_read_off; uint32_t* out_cigars; int64_t* out_cigar_off;
    int64_t* out_ref_start; uint8_t* out_mapq; int8_t* out_orientation; uint8_t* out_hp; int32_t* out_site;
    int64_t n_reads, read_shift, base_shift, cigar_shift;
    int32_t site_shift;
};

// One wave per output read: the lanes copy the read's bases, qualities and CIGAR words to [base_shift + base_off[i], ...) /
// [cigar_shift + cigar_off[i], ...) byte by byte and word by word (offsets on either side are arbitrary; nothing outside the
// read's own range is touched); lane 0 writes the per-read entries at read_shift + i and the offsets behind it.  Every output
// element has one writer.
__global__ __launch_bounds__(256) void gather_reads_kernel(GatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n_reads) return;
    const int64_t r = a.source[i];
    const int64_t b0 = a.t_base_off[i], b1 = a.t_base_off[i + 1], c0 = a.t_cigar_off[i], c1 = a.t_cigar_off[i + 1];
    if (r >= 0) {
        const int64_t src = a.read_off[r], dst = a.base_shift + b0, n_bases = b1 - b0;
        for (int64_t k = lane; k < n_bases; k += 64) {
            a.out_bases[dst + k] = a.bases[src + k];
            a.out_quals[dst + k] = a.quals[src + k];
        }
        const int64_t csrc = a.cigar_off[r], cdst = a.cigar_shift + c0, n_ops = c1 - c0;
        for (int64_t k = lane; k < n_ops; k += 64) a.out_cigars[cdst + k] = a.cigars[csrc + k];
    }
    if (lane == 0) {
        const int64_t o = a.read_shift + i;
        if (i == 0) {
            a.out_read_off[o] = a.base_shift;
            a.out_cigar_off[o] = a.cigar_shift;
        }
        a.out_read_off[o + 1] = a.base_shift + b1;
        a.out_cigar_off[o + 1] = a.cigar_shift + c1;
        a.out_ref_start[o] = r >= 0 ? a.ref_start[r] : 0;                    // the dummy read of featurizer_core
        a.out_mapq[o] = r >= 0 ? a.mapq[r] : (uint8_t)40;
        a.out_orientation[o] = r >= 0 ? a.orientation[r] : (int8_t)1;
        a.out_hp[o] = r >= 0 ? a.hp[r] : (uint8_t)0;
        a.out_site[o] = a.site[i] + a.site_shift;
    }
}

template <class T> const T* device_copy(DevMem& m, const T* from, size_t n) {       // device to device
    void* p = nullptr;
    HS_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    m.ptrs.push_back(p);
    if (n) HS_HIP(hipMemcpy(p, from, n * sizeof(T), hipMemcpyDeviceToDevice));
    return (const T*)p;
}

// HELLO_CANDIDATES_RESIDENT instead of gather_reads: rs2's device arrays are copied on the device into memory the result
// owns (the call's own allocations -- the chromosome, the kernels' scratch, pass 1 -- are freed when it returns), the gather
// table of every technology is uploaded, and read_index is turned into input reads as gather_reads does.  Reads below
// `n_first` of rs2 take orientation and hp from flags0 / hp0, the others from flags1 / hp1.
void keep_resident(hello_candidates& o, const ReadSet& rs2, int64_t n_first, const uint16_t* flags0, const uint8_t* hp0,
                   const uint16_t* flags1, const uint8_t* hp1) {
    o.resident = true;
    hello_candidates* tech[2] = {&o, o.second.get()};
    if (!o.start.empty()) {
        auto res = std::make_unique<Resident>();
        DevMem& m = res->mem;
        const size_t n = (size_t)rs2.n;
        res->bases = device_copy(m, rs2.d.bases, (size_t)rs2.read_off[n]);
        res->quals = device_copy(m, rs2.d.quals, (size_t)rs2.read_off[n]);
        res->read_off = device_copy(m, rs2.d.read_off, n + 1);
        res->cigars = device_copy(m, rs2.d.cigars, (size_t)rs2.cigar_off[n]);
        res->cigar_off = device_copy(m, rs2.d.cigar_off, n + 1);
        res->ref_start = device_copy(m, rs2.d.ref_start, n);
        res->mapq = m.put(rs2.mapq, n);
        std::vector<int8_t> orientation(n);
        std::vector<uint8_t> hp(n);
        for (int64_t r = 0; r < rs2.n; ++r) {
            const int64_t in = rs2.input(r);
            orientation[r] = ((r < n_first ? flags0 : flags1)[in] & 16) ? -1 : 1;
            hp[r] = (r < n_first ? hp0 : hp1)[in];
        }
        res->orientation = m.put(orientation.data(), n);
        res->hp = m.put(hp.data(), n);
        for (int t = 0; t < 2 && tech[t]; ++t) {
            GatherTable table;
            table.build(tech[t]->reads_per_allele.data(), (int64_t)tech[t]->reads_per_allele.size(), tech[t]->read_off.data(),
                        tech[t]->cigar_off.data(), o.alleles_per_site.data(), (int64_t)o.alleles_per_site.size());
            for (int64_t& s : table.source)
                if (s >= 0) s = tech[t]->read_index[s];                     // the read of rs2
            res->table[t].source = m.put(table.source.data(), table.source.size());
            res->table[t].base_off = m.put(table.base_off.data(), table.base_off.size());
            res->table[t].cigar_off = m.put(table.cigar_off.data(), table.cigar_off.size());
            res->table[t].site = m.put(table.site.data(), table.site.size());
        }
        HS_HIP(hipStreamSynchronize(0));       // the copies are complete before a gather on another stream reads them
        o.on_device = std::move(res);
    }
    for (int t = 0; t < 2 && tech[t]; ++t)
        for (int64_t& r : tech[t]->read_index) r = rs2.input(r);
}

// The sizes of a technology's featurizer input, dummy reads included.
void featurizer_counts(const hello_candidates& c, int64_t& n_reads, int64_t& n_bases, int64_t& n_cigars) {
    n_reads = 0;
    for (int32_t n : c.reads_per_allele) n_reads += std::max(n, 1);
    n_bases = c.read_off.back();
    n_cigars = c.cigar_off.back();
}

// ---- two BAMs

// One pass's reads of both technologies as one set: the Illumina input reads, then the clipped PacBio copies (table 1).
void join_sets(const ReadSet& ill, const ReadSet& clipped, ReadSet& out) {
    const int64_t ni = ill.n, np = clipped.n;
    auto cat = [](auto& to, const auto* x, int64_t nx, const auto* y, int64_t ny) {
        to.assign(x, x + nx);
        to.insert(to.end(), y, y + ny);
    };
    auto cat_off = [](std::vector<int64_t>& to, const int64_t* x, int64_t nx, const int64_t* y, int64_t ny) {
        to.assign(x, x + nx + 1);
        for (int64_t i = 1; i <= ny; ++i) to.push_back(x[nx] + y[i]);
    };
    out.n = ni + np;
    cat(out.v_bases, ill.bases, ill.read_off[ni], clipped.bases, clipped.read_off[np]);
    cat(out.v_quals, ill.quals, ill.read_off[ni], clipped.quals, clipped.read_off[np]);
    cat(out.v_cigars, ill.cigars, ill.cigar_off[ni], clipped.cigars, clipped.cigar_off[np]);
    cat_off(out.v_read_off, ill.read_off, ni, clipped.read_off, np);
    cat_off(out.v_cigar_off, ill.cigar_off, ni, clipped.cigar_off, np);
    cat(out.v_ref_start, ill.ref_start, ni, clipped.ref_start, np);
    cat(out.v_ref_end, ill.ref_end, ni, clipped.ref_end, np);
    cat(out.v_mapq, ill.mapq, ni, clipped.mapq, np);
    out.v_origin.resize((size_t)(ni + np));
    for (int64_t r = 0; r < ni; ++r) out.v_origin[r] = r;
    for (int64_t r = 0; r < np; ++r) out.v_origin[ni + r] = clipped.origin[r];
    cat_off(out.plant_off, ill.plant_off.data(), ni, clipped.plant_off.data(), np);
    cat(out.plant, ill.plant.data(), (int64_t)ill.plant.size(), clipped.plant.data(), (int64_t)clipped.plant.size());
    cat(out.last_pos, ill.last_pos.data(), ni, clipped.last_pos.data(), np);
    cat(out.pflags, ill.pflags.data(), ni, clipped.pflags.data(), np);
    out.bases = out.v_bases.data(); out.quals = out.v_quals.data(); out.read_off = out.v_read_off.data();
    out.cigars = out.v_cigars.data(); out.cigar_off = out.v_cigar_off.data(); out.ref_start = out.v_ref_start.data();
    out.ref_end = out.v_ref_end.data(); out.mapq = out.v_mapq.data(); out.origin = out.v_origin.data();
    std::vector<uint8_t> table((size_t)(ni + np), 0);
    std::fill(table.begin() + ni, table.end(), (uint8_t)1);
    out.d = upload_reads(out.mem, out);
    out.d_ref_end = out.mem.put(out.ref_end, out.v_ref_end.size());
    out.d_table = out.mem.put(table.data(), table.size());
}

// The coverage gate of a cluster (python/AlleleSearcherLite.py:264-266: container 0's average_coverage > 14; DESIGN.md "Two
// BAMs" defines the rule): over the Illumina reads that overlap [lo, hi) and are mapped, primary, not QC-fail, not duplicate and
// a proper pair if paired -- before de-duplication and the cap -- sum of counts > 14 * columns.
bool coverage_gate(const ReadsView& in, int64_t max_span, int64_t lo, int64_t hi) {
    const int64_t* begin = in.ref_start;
    const int64_t first = std::lower_bound(begin, begin + in.n, lo - max_span) - begin;
    // first walk: the reads that count, checked once (they include reads the searchers skip and strict_walk did not look
    // at), and the span of their columns
    std::vector<int64_t> counted;
    int64_t c_lo = INT64_MAX, c_hi = INT64_MIN;
    for (int64_t r = first; r < in.n && in.ref_start[r] < hi; ++r) {
        const uint16_t f = in.flags[r];
        if (in.ref_end[r] <= lo || (f & (0x4 | 0x100 | 0x800 | 0x200 | 0x400)) || ((f & 0x1) && !(f & 0x2))) continue;
        int64_t qlen = 0, rlen = 0;
        for (int64_t c = in.cigar_off[r]; c < in.cigar_off[r + 1]; ++c) {
            const int op = in.cigars[c] & 15;
            if (op > 8) raise(HELLO_ERR_ARG, "read %lld: CIGAR operation %d", (long long)r, op);
            if (is_query_op(op)) qlen += in.cigars[c] >> 4;
            if (is_ref_op(op)) rlen += in.cigars[c] >> 4;
        }
        if (qlen != in.read_off[r + 1] - in.read_off[r])
            raise(HELLO_ERR_SHAPE, "read %lld: CIGAR query length %lld, %lld bases", (long long)r, (long long)qlen,
                  (long long)(in.read_off[r + 1] - in.read_off[r]));
        counted.push_back(r);
        c_lo = std::min(c_lo, in.ref_start[r]);
        c_hi = std::max(c_hi, in.ref_start[r] + rlen);
    }
    if (c_lo >= c_hi) return false;                                  // no column: 0 > 0 is false
    std::vector<uint8_t> column((size_t)(c_hi - c_lo), 0);
    int64_t total = 0;
    for (int64_t r : counted) {
        const bool good = in.mapq[r] >= 10;
        const uint8_t* quals = in.quals + in.read_off[r];
        int64_t rf = in.ref_start[r], rd = 0;
        for (int64_t c = in.cigar_off[r]; c < in.cigar_off[r + 1]; ++c) {
            const int op = in.cigars[c] & 15;
            const int64_t n = in.cigars[c] >> 4;
            if (op == 0 || op == 7 || op == 8) {
                for (int64_t j = 0; j < n; ++j) {
                    column[(size_t)(rf + j - c_lo)] = 1;
                    total += good && quals[rd + j] >= 13;
                }
                rf += n; rd += n;
            } else if (op == 2 || op == 3) {                          // the quality of the last read base before the operation
                std::fill(column.begin() + (rf - c_lo), column.begin() + (rf + n - c_lo), (uint8_t)1);
                if (good && rd > 0 && quals[rd - 1] >= 13) total += n;
                rf += n;
            } else if (op == 1 || op == 4) {
                rd += n;
            }
        }
    }
    int64_t columns = 0;
    for (uint8_t c : column) columns += c;
    return total > 14 * columns;
}

}  // namespace
}  // namespace hello

extern "C" {

int hello_candidates_find(const uint8_t* bases, const uint8_t* quals, const int64_t* read_offsets, const uint32_t* cigars,
                          const int64_t* cigar_offsets, const int64_t* ref_starts, const int64_t* ref_ends, const uint8_t* mapq,
                          const uint16_t* flags, const uint64_t* name_hash, const uint8_t* hp, int64_t n_reads,
                          const uint8_t* reference, int64_t reference_length, const int64_t* positions, int64_t n_positions,
                          int32_t options, int32_t feature_length, int32_t q_threshold, int32_t mapq_threshold, int32_t device,
                          hello_candidates** out) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    if (!out || !read_offsets || !cigar_offsets || (n_reads > 0 && (!bases || !quals || !cigars || !ref_starts || !ref_ends ||
        !mapq || !flags || !name_hash || !hp)) || !reference || (n_positions > 0 && !positions))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    if (n_reads < 0 || n_positions < 0 || reference_length < 0 || feature_length <= 0)
        return set_last_error(HELLO_ERR_ARG, "negative count");
    if (options & (HELLO_HOTSPOTS_TWO_BAMS | HELLO_HOTSPOTS_HYBRID))
        return set_last_error(HELLO_ERR_ARG, "candidate sites are built from one Illumina BAM: PacBio reads, two BAMs and hybrid "
                                             "hotspots need the PacBio reassembly and read clipping, which this library does not have");
    if (options & ~(HELLO_HOTSPOTS_PACBIO | HELLO_CANDIDATES_RESIDENT)) return set_last_error(HELLO_ERR_ARG, "options %d", options);
    const bool pacbio = (options & HELLO_HOTSPOTS_PACBIO) != 0, resident = (options & HELLO_CANDIDATES_RESIDENT) != 0;
    for (int64_t i = 1; i < n_positions; ++i)
        if (positions[i] < positions[i - 1]) return set_last_error(HELLO_ERR_ARG, "position %lld: positions are not sorted", (long long)i);

    const ReadsView in{bases, quals, read_offsets, cigars, cigar_offsets, ref_starts, ref_ends, mapq, flags, name_hash, n_reads};
    ReadSet input;                                     // strict_walk: validation, planting positions, last_position, partials
    static_cast<ReadsView&>(input) = in;
    strict_walk(in, pacbio ? kStrictClipInput : kStrictRegions, input);
    const int64_t max_span = input.max_span[0];

    std::vector<Job> jobs1 = active_region_jobs(positions, n_positions);
    auto res = std::make_unique<hello_candidates>();
    res->resident = resident;
    JobStats st1, st2;
    float allele_ms = 0.0f;
    double ms_gather = 0.0;
    int64_t n_slots = 0, n_clusters = 0, sites_oob = 0;
    if (n_reads == 0) st1.empty = (int64_t)jobs1.size();
    if (!jobs1.empty() && n_reads > 0) {
        open_device(device);
        DevMem m;
        HotspotArgs a{};
        std::vector<uint8_t> table(n_reads, 0);                      // every read counts in the Illumina table
        input.d = upload_reads(m, in);
        input.d_ref_end = m.put(ref_ends, (size_t)n_reads);
        input.d_table = m.put(table.data(), table.size());
        ReadSet clipped1, clipped2;                                  // PacBio: the clipped reads of pass 1 and of pass 2
        a.ref_lo = 0;
        a.ref_len = reference_length;
        a.ref = m.put(reference, (size_t)reference_length);
        a.q_threshold = q_threshold;
        a.hybrid = 0;

        select_reads(jobs1, in, max_span, pacbio, st1);
        if (pacbio) clip_reads(jobs1, in, input, clipped1, st1);
        differing_regions(jobs1, pacbio ? clipped1 : input, reference_length, mapq_threshold, a, st1);
        const auto locations = pass1_locations(jobs1, *res);

        std::vector<Job> jobs2 = cluster_jobs(locations);
        n_clusters = (int64_t)jobs2.size();
        select_reads(jobs2, in, max_span, pacbio, st2);                // a fresh fetch from the input reads (trainDataTools.py:1059-1065)
        if (pacbio) clip_reads(jobs2, in, input, clipped2, st2);
        const ReadSet& rs2 = pacbio ? clipped2 : input;              // the reads of the clusters, of the alleles and of the shard
        differing_regions(jobs2, rs2, reference_length, mapq_threshold, a, st2);

        AllelePlan plan;
        plan.build(jobs2, rs2, *res);
        n_slots = plan.n_slots;
        AlleleResult got(plan);
        if (plan.n_cl > 0 && n_slots > 0) {
            const AlleleArgs b = plan.upload(m, rs2, a.ref, reference_length, q_threshold, mapq_threshold);
            {
                KernelTimer timer;
                timer.start();
                hipLaunchKernelGGL(allele_kernel, dim3((unsigned)plan.n_cl), dim3(256), 0, 0, b);
                allele_ms = timer.stop();
            }
            got.download(b);
        }

        const auto tg = clock::now();
        sites_oob = emit_sites(*res, nullptr, plan, got, rs2, reference, reference_length, feature_length);
        if (resident) {
            keep_resident(*res, rs2, rs2.n, flags, hp, flags, hp);
        } else {
            gather_reads(*res, rs2, flags, hp);
            ms_gather = std::chrono::duration<double, std::milli>(clock::now() - tg).count();
        }
    }
    const double ms_total = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    const double st[HELLO_CANDIDATES_STATS] = {
        (double)jobs1.size(), (double)st1.empty, (double)st1.bounds, (double)st1.capped, (double)(res->regions1.size() / 2),
        (double)n_clusters, (double)st2.empty, (double)st2.bounds, (double)st2.capped, (double)(res->regions2.size() / 2),
        (double)res->start.size(), (double)sites_oob, (double)res->reads_per_allele.size(), (double)res->read_index.size(),
        (double)n_slots, (double)st1.ms, (double)st2.ms, (double)allele_ms, ms_gather, ms_total,
        (double)st1.clip_ms + (double)st2.clip_ms, (double)(st1.clipped + st2.clipped)};
    std::copy(st, st + HELLO_CANDIDATES_STATS, res->stats);
    *out = res.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_candidates_find")

int hello_candidates_find_hybrid(
    const uint8_t* bases0, const uint8_t* quals0, const int64_t* read_offsets0, const uint32_t* cigars0, const int64_t* cigar_offsets0,
    const int64_t* ref_starts0, const int64_t* ref_ends0, const uint8_t* mapq0, const uint16_t* flags0, const uint64_t* name_hash0,
    const uint8_t* hp0, int64_t n_reads0,
    const uint8_t* bases1, const uint8_t* quals1, const int64_t* read_offsets1, const uint32_t* cigars1, const int64_t* cigar_offsets1,
    const int64_t* ref_starts1, const int64_t* ref_ends1, const uint8_t* mapq1, const uint16_t* flags1, const uint64_t* name_hash1,
    const uint8_t* hp1, int64_t n_reads1,
    const uint8_t* reference, int64_t reference_length, const int64_t* positions, int64_t n_positions, int32_t options,
    int32_t reassembly_size, int32_t feature_length, int32_t q_threshold, int32_t mapq_threshold, int32_t device,
    hello_candidates** out) try {
    using namespace hello;
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    auto missing = [](int64_t n, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, const void* g,
                      const void* h, const void* i) { return n > 0 && (!a || !b || !c || !d || !e || !f || !g || !h || !i); };
    if (!out || !read_offsets0 || !cigar_offsets0 || !read_offsets1 || !cigar_offsets1 || !reference || (n_positions > 0 && !positions) ||
        missing(n_reads0, bases0, quals0, cigars0, ref_starts0, ref_ends0, mapq0, flags0, name_hash0, hp0) ||
        missing(n_reads1, bases1, quals1, cigars1, ref_starts1, ref_ends1, mapq1, flags1, name_hash1, hp1))
        return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    if (n_reads0 < 0 || n_reads1 < 0 || n_positions < 0 || reference_length < 0 || feature_length <= 0)
        return set_last_error(HELLO_ERR_ARG, "negative count");
    if (options & ~(HELLO_HOTSPOTS_HYBRID | HELLO_CANDIDATES_RESIDENT))
        return set_last_error(HELLO_ERR_ARG, "options %d: HELLO_HOTSPOTS_HYBRID and HELLO_CANDIDATES_RESIDENT are understood", options);
    const bool resident = (options & HELLO_CANDIDATES_RESIDENT) != 0;
    for (int64_t i = 1; i < n_positions; ++i)
        if (positions[i] < positions[i - 1]) return set_last_error(HELLO_ERR_ARG, "position %lld: positions are not sorted", (long long)i);

    const ReadsView in0{bases0, quals0, read_offsets0, cigars0, cigar_offsets0, ref_starts0, ref_ends0, mapq0, flags0, name_hash0, n_reads0};
    const ReadsView in1{bases1, quals1, read_offsets1, cigars1, cigar_offsets1, ref_starts1, ref_ends1, mapq1, flags1, name_hash1, n_reads1};
    ReadSet input0, input1;
    static_cast<ReadsView&>(input0) = in0;
    static_cast<ReadsView&>(input1) = in1;
    strict_walk(in0, kStrictRegions, input0);
    strict_walk(in1, kStrictClipInput, input1);
    const int64_t max_span0 = input0.max_span[0], max_span1 = input1.max_span[0];
    int64_t max_span_all0 = 0;                         // the coverage gate looks at reads the searchers do not use
    for (int64_t r = 0; r < n_reads0; ++r) max_span_all0 = std::max(max_span_all0, ref_ends0[r] - ref_starts0[r]);

    std::vector<Job> jobs1 = active_region_jobs(positions, n_positions);
    auto res = std::make_unique<hello_candidates>();
    res->second = std::make_unique<hello_candidates>();
    res->resident = resident;
    JobStats st1, st2;
    float allele_ms = 0.0f, reassembly_ms = 0.0f;
    double ms_gather = 0.0;
    int64_t n_slots = 0, n_clusters = 0, sites_oob = 0;
    int64_t gate_passed = 0, reassembled = 0, eligible = 0, reassigned = 0, by_tie = 0, illumina_sites = 0;
    if (n_reads0 + n_reads1 == 0) st1.empty = (int64_t)jobs1.size();
    if (!jobs1.empty() && n_reads0 + n_reads1 > 0) {
        open_device(device);
        DevMem m;
        HotspotArgs a{};
        input1.d = upload_reads(m, in1);                                          // what the clip kernels read
        input1.d_ref_end = m.put(ref_ends1, (size_t)n_reads1);
        a.ref_lo = 0;
        a.ref_len = reference_length;
        a.ref = m.put(reference, (size_t)reference_length);
        a.q_threshold = q_threshold;
        a.hybrid = (options & HELLO_HOTSPOTS_HYBRID) ? 1 : 0;

        // A pass: every searcher's two containers (AlleleSearcherLite.py:116-127), selected and capped each on its own; the
        // PacBio container's reads clipped; both as one read list with a table byte per read for the differing-position kernel.
        ReadSet clipped1, clipped2, both1, both2;
        auto pass = [&](std::vector<Job>& jobs, ReadSet& clipped, ReadSet& both, JobStats& st) {
            std::vector<Job> container1 = jobs;                      // the same searchers' PacBio containers
            JobStats each;
            select_reads(jobs, in0, max_span0, false, each);
            select_reads(container1, in1, max_span1, true, each);
            clip_reads(container1, in1, input1, clipped, st);
            join_sets(input0, clipped, both);
            for (size_t j = 0; j < jobs.size(); ++j) {
                for (int64_t r : container1[j].reads) jobs[j].reads.push_back(n_reads0 + r);
                jobs[j].capped = jobs[j].capped || container1[j].capped;
                if (jobs[j].reads.empty()) ++st.empty;               // all(self.noReads): no regions
            }
            differing_regions(jobs, both, reference_length, mapq_threshold, a, st);
        };
        pass(jobs1, clipped1, both1, st1);
        const auto locations = pass1_locations(jobs1, *res);
        std::vector<Job> jobs2 = cluster_jobs(locations);
        n_clusters = (int64_t)jobs2.size();
        pass(jobs2, clipped2, both2, st2);
        const ReadSet& rs2 = both2;

        std::vector<uint8_t> gate(jobs2.size(), 0);
        for (size_t j = 0; j < jobs2.size(); ++j)
            if (jobs2[j].run) {
                gate[j] = coverage_gate(in0, max_span_all0, jobs2[j].fetch_lo, jobs2[j].fetch_hi) ? 1 : 0;
                gate_passed += gate[j];
            }

        AllelePlan plan;
        plan.build(jobs2, rs2, *res);
        n_slots = plan.n_slots;
        AlleleResult got(plan);
        if (plan.n_cl > 0 && n_slots > 0) {
            AlleleArgs b = plan.upload(m, rs2, a.ref, reference_length, q_threshold, mapq_threshold);
            b.tech = rs2.d_table;
            b.alias = m.zeros<int64_t>((size_t)n_slots);
            HS_HIP(hipMemset(b.alias, 0xFF, (size_t)n_slots * sizeof(int64_t)));                 // -1
            b.reassigned = m.zeros<uint8_t>(plan.cl_reads.size());
            b.site_al = m.zeros<int64_t>((size_t)n_slots);
            b.n_site_al = m.zeros<int32_t>((size_t)plan.n_reg);
            b.al_count1 = m.zeros<int32_t>((size_t)n_slots);
            {
                KernelTimer timer;
                timer.start();
                hipLaunchKernelGGL(hybrid_records_kernel, dim3((unsigned)plan.n_cl), dim3(256), 0, 0, b);
                allele_ms = timer.stop();
            }

            // ---- reassembly plan: the (cluster, eligible PacBio read) pairs and their scratch, counted from the records
            const auto tr = clock::now();
            std::vector<int32_t> status((size_t)n_slots), len((size_t)n_slots), n_site_al((size_t)plan.n_reg);
            fetch(status, b.status);
            fetch(len, b.len);
            fetch(n_site_al, b.n_site_al);
            std::vector<int64_t> pair_x, pair_c, hap_off{0}, bit_off{0};
            for (int64_t c = 0; c < plan.n_cl; ++c) {
                const int64_t g0 = plan.cl_reg_off[c], g1 = plan.cl_reg_off[c + 1], ng = g1 - g0;
                if (!gate[plan.cl_job[c]] || ng >= reassembly_size) continue;                    // :695
                ++reassembled;
                for (int64_t g = g0; g < g1; ++g) illumina_sites += n_site_al[g] > 0;
                const int64_t start = plan.reg_start[g0] - 6, stop = plan.reg_stop[g1 - 1] + 6;  // band_margin (:682-683)
                for (int64_t x = plan.cl_read_off[c]; x < plan.cl_read_off[c + 1]; ++x) {
                    const int64_t r = plan.cl_reads[x];
                    if (r < n_reads0 || rs2.ref_start[r] > start || rs2.last_pos[r] < stop) continue;    // spans it (Read.cpp:211-214)
                    const int64_t s0 = plan.rd_rec_off[x];
                    if (plan.rd_rec_off[x + 1] - s0 != ng || start < 0 || stop > reference_length)
                        raise(HELLO_ERR_ARG, "internal: a spanning read without a record in every region");
                    int64_t H = stop - start;
                    for (int64_t g = g0; g < g1; ++g)
                        if (status[s0 + g - g0] == kSuccess) H += len[s0 + g - g0] - (plan.reg_stop[g] - plan.reg_start[g]);
                    pair_x.push_back(x);
                    pair_c.push_back(c);
                    hap_off.push_back(hap_off.back() + H);
                    bit_off.push_back(bit_off.back() + (ng + 1) * ((H + 1 + 31) / 32));
                }
            }
            eligible = (int64_t)pair_x.size();
            if (eligible > 0) {
                ReassemblyArgs q{};
                q.a = b;
                q.pair_x = m.put(pair_x.data(), pair_x.size());
                q.pair_c = m.put(pair_c.data(), pair_c.size());
                q.hap_off = m.put(hap_off.data(), hap_off.size());
                q.bit_off = m.put(bit_off.data(), bit_off.size());
                q.hap = m.zeros<uint8_t>((size_t)hap_off.back());
                q.bits = m.zeros<unsigned>((size_t)bit_off.back());
                q.result = m.zeros<int32_t>((size_t)eligible);
                q.n_pairs = eligible;
                hipLaunchKernelGGL(reassemble_kernel, dim3((unsigned)eligible), dim3(64), 0, 0, q);
                HS_HIP(hipGetLastError());
                std::vector<int32_t> result((size_t)eligible);
                fetch(result, (const int32_t*)q.result);
                for (int32_t v : result) {
                    if (v < 0) raise(HELLO_ERR_ARG, "internal: reassembly scratch (%d)", v);
                    reassigned += v > 0;
                    by_tie += v == 2;
                }
            }
            reassembly_ms = (float)std::chrono::duration<double, std::milli>(clock::now() - tr).count();
            {
                KernelTimer timer;
                timer.start();
                hipLaunchKernelGGL(hybrid_alleles_kernel, dim3((unsigned)plan.n_cl), dim3(256), 0, 0, b);
                allele_ms += timer.stop();
            }
            got.download(b);
        } else {
            got.al_count1.resize(got.al_count.size());
        }

        const auto tg = clock::now();
        sites_oob = emit_sites(*res, res->second.get(), plan, got, rs2, reference, reference_length, feature_length);
        if (resident) {
            keep_resident(*res, rs2, n_reads0, flags0, hp0, flags1, hp1);
        } else {
            gather_reads(*res, rs2, flags0, hp0);
            gather_reads(*res->second, rs2, flags1, hp1);
            ms_gather = std::chrono::duration<double, std::milli>(clock::now() - tg).count();
        }
    }
    const double ms_total = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    const double st[HELLO_CANDIDATES_STATS] = {
        (double)jobs1.size(), (double)st1.empty, (double)st1.bounds, (double)st1.capped, (double)(res->regions1.size() / 2),
        (double)n_clusters, (double)st2.empty, (double)st2.bounds, (double)st2.capped, (double)(res->regions2.size() / 2),
        (double)res->start.size(), (double)sites_oob, (double)res->reads_per_allele.size(),
        (double)(res->read_index.size() + res->second->read_index.size()),
        (double)n_slots, (double)st1.ms, (double)st2.ms, (double)allele_ms, ms_gather, ms_total,
        (double)st1.clip_ms + (double)st2.clip_ms, (double)(st1.clipped + st2.clipped)};
    std::copy(st, st + HELLO_CANDIDATES_STATS, res->stats);
    const double hst[HELLO_CANDIDATES_HYBRID_STATS - HELLO_CANDIDATES_STATS] = {
        (double)gate_passed, (double)reassembled, (double)eligible, (double)reassigned, (double)by_tie, (double)illumina_sites,
        (double)reassembly_ms};
    std::copy(hst, hst + (HELLO_CANDIDATES_HYBRID_STATS - HELLO_CANDIDATES_STATS), res->hybrid_stats);
    *out = res.release();
    return HELLO_OK;
} HS_ENTRY_END("hello_candidates_find_hybrid")

int hello_candidates_array(const hello_candidates* c, int32_t which, const void** data, int64_t* count) {
    if (!c || !data || !count) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
#define HELLO_CAND_CASE(id, v) case id: *data = c->v.data(); *count = (int64_t)c->v.size(); break
    switch (which) {
        HELLO_CAND_CASE(HELLO_CAND_START, start);
        HELLO_CAND_CASE(HELLO_CAND_STOP, stop);
        HELLO_CAND_CASE(HELLO_CAND_WINDOW_START, window_start);
        HELLO_CAND_CASE(HELLO_CAND_REF_OFF, ref_off);
        HELLO_CAND_CASE(HELLO_CAND_REF, ref);
        HELLO_CAND_CASE(HELLO_CAND_ALLELES_PER_SITE, alleles_per_site);
        HELLO_CAND_CASE(HELLO_CAND_ALLELE_TEXT, allele_text);
        HELLO_CAND_CASE(HELLO_CAND_ALLELE_TEXT_OFF, allele_text_off);
        HELLO_CAND_CASE(HELLO_CAND_READS_PER_ALLELE, reads_per_allele);
        HELLO_CAND_CASE(HELLO_CAND_BASES, bases);
        HELLO_CAND_CASE(HELLO_CAND_QUALS, quals);
        HELLO_CAND_CASE(HELLO_CAND_READ_OFF, read_off);
        HELLO_CAND_CASE(HELLO_CAND_CIGARS, cigars);
        HELLO_CAND_CASE(HELLO_CAND_CIGAR_OFF, cigar_off);
        HELLO_CAND_CASE(HELLO_CAND_REF_START, ref_start);
        HELLO_CAND_CASE(HELLO_CAND_MAPQ, mapq);
        HELLO_CAND_CASE(HELLO_CAND_ORIENTATION, orientation);
        HELLO_CAND_CASE(HELLO_CAND_HP, hp);
        HELLO_CAND_CASE(HELLO_CAND_READ_INDEX, read_index);
        HELLO_CAND_CASE(HELLO_CAND_REGIONS_PASS1, regions1);
        HELLO_CAND_CASE(HELLO_CAND_REGIONS_PASS2, regions2);
        default: return hello::set_last_error(HELLO_ERR_ARG, "no candidate array %d", which);
    }
#undef HELLO_CAND_CASE
    return HELLO_OK;
}

int hello_candidates_stats(const hello_candidates* c, double* stats) {
    if (!c || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(c->stats, c->stats + HELLO_CANDIDATES_STATS, stats);
    return HELLO_OK;
}

int hello_candidates_array_tech(const hello_candidates* c, int32_t tech, int32_t which, const void** data, int64_t* count) {
    if (!c || !data || !count) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (tech == 0) return hello_candidates_array(c, which, data, count);
    if (tech != 1 || !c->second) return hello::set_last_error(HELLO_ERR_ARG, "no technology %d in these candidates", tech);
    if (which < HELLO_CAND_READS_PER_ALLELE || which > HELLO_CAND_READ_INDEX)
        return hello::set_last_error(HELLO_ERR_ARG, "candidate array %d is not a read array of a technology", which);
    return hello_candidates_array(c->second.get(), which, data, count);
}

int hello_candidates_hybrid_stats(const hello_candidates* c, double* stats) {
    if (!c || !stats) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    std::copy(c->stats, c->stats + HELLO_CANDIDATES_STATS, stats);
    std::copy(c->hybrid_stats, c->hybrid_stats + (HELLO_CANDIDATES_HYBRID_STATS - HELLO_CANDIDATES_STATS), stats + HELLO_CANDIDATES_STATS);
    return HELLO_OK;
}

void hello_candidates_free(hello_candidates* c) { delete c; }

int hello_candidates_featurizer_counts(const hello_candidates* c, int32_t tech, int64_t* n_reads, int64_t* n_bases, int64_t* n_cigars) {
    if (!c || !n_reads || !n_bases || !n_cigars) return hello::set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (tech != 0 && (tech != 1 || !c->second)) return hello::set_last_error(HELLO_ERR_ARG, "no technology %d in these candidates", tech);
    hello::featurizer_counts(tech ? *c->second : *c, *n_reads, *n_bases, *n_cigars);
    return HELLO_OK;
}

int hello_candidates_gather(const hello_candidates* c, int32_t tech, uint8_t* bases, uint8_t* quals, int64_t* read_off, uint32_t* cigars,
                            int64_t* cigar_off, int64_t* ref_start, uint8_t* mapq, int8_t* orientation, uint8_t* hp,
                            int32_t* site_of_read, int64_t read_shift, int64_t base_shift, int64_t cigar_shift, int64_t site_shift,
                            void* hip_stream) try {
    using namespace hello;
    if (!c) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (!c->resident)
        return set_last_error(HELLO_ERR_ARG, "these candidates were not built with HELLO_CANDIDATES_RESIDENT: their reads are on the "
                                             "host (hello_candidates_array)");
    if (tech != 0 && (tech != 1 || !c->second)) return set_last_error(HELLO_ERR_ARG, "no technology %d in these candidates", tech);
    if (read_shift < 0 || base_shift < 0 || cigar_shift < 0 || site_shift < 0 || site_shift > INT32_MAX)
        return set_last_error(HELLO_ERR_ARG, "negative shift (read_shift %lld, base_shift %lld, cigar_shift %lld, site_shift %lld)",
                              (long long)read_shift, (long long)base_shift, (long long)cigar_shift, (long long)site_shift);
    int64_t n_reads = 0, n_bases = 0, n_cigars = 0;
    featurizer_counts(tech ? *c->second : *c, n_reads, n_bases, n_cigars);
    if (n_reads == 0) return HELLO_OK;
    if (!bases || !quals || !read_off || !cigars || !cigar_off || !ref_start || !mapq || !orientation || !hp || !site_of_read)
        return set_last_error(HELLO_ERR_ARG, "NULL destination for %lld reads", (long long)n_reads);
    if (!c->on_device) return set_last_error(HELLO_ERR_ARG, "internal: resident candidates with reads and no device memory");
    const Resident& d = *c->on_device;
    GatherArgs a{};
    a.bases = d.bases; a.quals = d.quals; a.read_off = d.read_off; a.cigars = d.cigars; a.cigar_off = d.cigar_off;
    a.ref_start = d.ref_start; a.mapq = d.mapq; a.orientation = d.orientation; a.hp = d.hp;
    a.source = d.table[tech].source; a.t_base_off = d.table[tech].base_off; a.t_cigar_off = d.table[tech].cigar_off;
    a.site = d.table[tech].site;
    a.out_bases = bases; a.out_quals = quals; a.out_read_off = read_off; a.out_cigars = cigars; a.out_cigar_off = cigar_off;
    a.out_ref_start = ref_start; a.out_mapq = mapq; a.out_orientation = orientation; a.out_hp = hp; a.out_site = site_of_read;
    a.n_reads = n_reads; a.read_shift = read_shift; a.base_shift = base_shift; a.cigar_shift = cigar_shift;
    a.site_shift = (int32_t)site_shift;
    hipLaunchKernelGGL(gather_reads_kernel, dim3((unsigned)((n_reads + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, a);
    HS_HIP(hipGetLastError());
    return HELLO_OK;
} HS_ENTRY_END("hello_candidates_gather")

int hello_candidates_gather_table(const int32_t* reads_per_allele, int64_t n_alleles, const int64_t* read_off, const int64_t* cigar_off,
                                  int64_t capacity, int64_t* source, int64_t* out_read_off, int64_t* out_cigar_off, int64_t* n_reads) try {
    using namespace hello;
    if (!n_reads || !read_off || !cigar_off || (n_alleles > 0 && !reads_per_allele)) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_alleles < 0 || capacity < 0) return set_last_error(HELLO_ERR_ARG, "negative count");
    for (int64_t k = 0; k < n_alleles; ++k)
        if (reads_per_allele[k] < 0) return set_last_error(HELLO_ERR_ARG, "allele %lld: negative reads_per_allele", (long long)k);
    GatherTable t;
    t.build(reads_per_allele, n_alleles, read_off, cigar_off, nullptr, 0);
    *n_reads = (int64_t)t.source.size();
    if (!source && !out_read_off && !out_cigar_off) return HELLO_OK;                 // the size only
    if ((!source && *n_reads > 0) || !out_read_off || !out_cigar_off) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (capacity < *n_reads) return set_last_error(HELLO_ERR_ARG, "capacity %lld for %lld reads", (long long)capacity, (long long)*n_reads);
    std::copy(t.source.begin(), t.source.end(), source);
    std::copy(t.base_off.begin(), t.base_off.end(), out_read_off);
    std::copy(t.cigar_off.begin(), t.cigar_off.end(), out_cigar_off);
    return HELLO_OK;
} HS_ENTRY_END("hello_candidates_gather_table")

}  // extern "C"
