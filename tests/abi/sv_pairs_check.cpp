// The rules of the read pairs and the clipped ends -- pair_counted, mate_valid, sv_pair_classify, sv_clips, sv_library_of and
// sv_cluster_pairs of hello_amd/csrc/sv_pairs.h over the clusters of hello_amd/csrc/sv.h -- as a stand-alone host program: built by
// tests/test_sv_pairs.py with -fsanitize=address,undefined and run directly on a file the test writes (the hand cases, the stress
// and the fuzz of tests/sv_pairs_cases.py).  It prints what it finds; the test compares that with the restatement of hello_amd/sv.py.
//
// The host's walk and marking run too: every block's reads go as real CIGARs through sv_walk (cigar.h) and sv_pairs_mark, the text
// hello_sv_add_pairs runs before any launch, and only what they mark is classified or has its clips counted.
//
// Input, line by line:  P length own n_contigs min_size flank mapq_threshold cluster_gap len_ratio_percent min_support clip_min
// median lo hi / R ref_start flag mapq hp mate_tid mate_pos has_sa CIGAR (a read, in coordinate order; ref_end comes from the
// CIGAR) / X and the eight columns of a row of another kind / E (the end of one block: the span is the whole chromosome).
// Output per E: per read one line "S status bin clips" and, with a row, a line "G" with its eight columns; a line "H" with the
// library of the block's inner distances (or "H none"), a line "K" with the eighteen columns per candidate, and a line "E".  Every
// array is allocated at exactly its size, so that an index that leaves it is caught.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../hello_amd/csrc/sv_pairs.h"

using namespace hello;

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: sv_pairs_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) return 2;
    long long length = 0, own = 0, n_contigs = 1, min_size = 1, flank = 1, mapq_threshold = 0, gap = 0, percent = 100, support = 1, clip_min = 1;
    long long median = 0, lo = 0, hi = 0, n_reads = 0;
    std::vector<SvSig> rows;
    std::vector<int64_t> inner(kInnerBins, 0);
    std::vector<uint32_t> ops;
    std::vector<int64_t> read_off{0}, cigar_off{0}, sa_off{0}, starts, ends, mate_pos;
    std::vector<int32_t> mate_tid;
    std::vector<uint16_t> flags;
    std::vector<uint8_t> mapqs, hps;
    auto clear_reads = [&] {
        ops.clear(); starts.clear(); ends.clear(); mate_pos.clear(); mate_tid.clear(); flags.clear(); mapqs.clear(); hps.clear();
        read_off.assign(1, 0); cigar_off.assign(1, 0); sa_off.assign(1, 0);
    };
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        char kind = 0;
        f >> kind;
        if (kind == 'P') {
            f >> length >> own >> n_contigs >> min_size >> flank >> mapq_threshold >> gap >> percent >> support >> clip_min >> median >> lo >> hi;
            rows.clear();
            inner.assign(kInnerBins, 0);
            clear_reads();
        } else if (kind == 'R') {
            long long st = 0, flag = 0, mapq = 0, hp = 0, mt = 0, ms = 0, has_sa = 0;
            std::string cigar;
            f >> st >> flag >> mapq >> hp >> mt >> ms >> has_sa >> cigar;
            long long qlen = 0, rlen = 0;
            for (size_t i = 0; i < cigar.size();) {
                size_t j = i;
                while (j < cigar.size() && cigar[j] >= '0' && cigar[j] <= '9') ++j;
                const uint32_t n = (uint32_t)std::strtoul(cigar.substr(i, j - i).c_str(), nullptr, 10);
                const int op = (int)std::string("MIDNSHP=X").find(cigar[j]);
                ops.push_back(n << 4 | (uint32_t)op);
                if (is_query_op(op)) qlen += n;
                if (is_ref_op(op)) rlen += n;
                i = j + 1;
            }
            cigar_off.push_back((int64_t)ops.size());
            read_off.push_back(read_off.back() + qlen);
            starts.push_back(st);
            ends.push_back(st + std::max<long long>(rlen, 1));
            flags.push_back((uint16_t)flag);
            mapqs.push_back((uint8_t)mapq);
            hps.push_back((uint8_t)hp);
            mate_tid.push_back((int32_t)mt);
            mate_pos.push_back(ms);
            sa_off.push_back(sa_off.back() + has_sa);
            ++n_reads;
        } else if (kind == 'X') {
            long long v[8] = {0};
            for (long long& x : v) f >> x;
            rows.push_back(SvSig{v[1], v[4], v[5], (int32_t)v[2], (int32_t)v[3], (uint8_t)v[0], (uint8_t)v[6], (uint8_t)v[7], 0});
        } else if (kind == 'E') {
            const size_t n = starts.size();
            std::unique_ptr<uint8_t[]> bases(new uint8_t[(size_t)read_off.back()]);
            std::fill(bases.get(), bases.get() + read_off.back(), (uint8_t)'A');
            std::unique_ptr<uint32_t[]> cig(new uint32_t[ops.size()]);            // exactly its size
            std::copy(ops.begin(), ops.end(), cig.get());
            ReadsView view{bases.get(), bases.get(), read_off.data(), cig.get(), cigar_off.data(), starts.data(), ends.data(), mapqs.data(),
                           flags.data(), nullptr, (int64_t)n};
            SvLibrary lib;
            lib.median = (int32_t)median; lib.lo = (int32_t)lo; lib.hi = (int32_t)hi;
            const SvWalk walk = sv_walk(view, 0, (int)mapq_threshold, min_size);
            const SvPairMarks marks = sv_pairs_mark(view, walk.kind, sa_off.data(), mate_tid.data(), mate_pos.data(), (int32_t)own, length,
                                                    (int)mapq_threshold, 0);
            for (size_t r = 0; r < n; ++r) {
                int status = marks.state[r], bin = -1, clips = 0;
                bool row = false;
                SvSig g{};
                if (marks.todo[r] & kPairClassify) {
                    const SvPairOutcome o = sv_pair_classify(flags[r], starts[r], ends[r], (int32_t)own, mate_tid[r], mate_pos[r], n_contigs, lib,
                                                             min_size);
                    status = o.status;
                    if (o.inner) { bin = o.bin; ++inner[(size_t)o.bin]; }
                    row = o.status == kPairRow || o.status == kPairBndRow;
                    g = SvSig{o.pos, marks.ordinal[r], kPairOp, (int32_t)o.len, (int32_t)o.shift, (uint8_t)o.type,
                              (uint8_t)((flags[r] & 0x10) ? 1 : 0), hps[r], 0};
                }
                if (marks.todo[r] & kPairClips) clips = sv_clips(cig.get() + cigar_off[r], cigar_off[r + 1] - cigar_off[r], clip_min);
                std::printf("S %d %d %d\n", status, bin, clips);
                if (row) {
                    std::printf("G %d %lld %d %d %lld %lld %d %d\n", g.type, (long long)g.pos, g.len, g.shift, (long long)g.ordinal,
                                (long long)g.op_index, g.strand, g.hp);
                    rows.push_back(g);
                }
            }
            int64_t lib3[3] = {0, 0, 0};
            if (sv_library_of(inner.data(), 8, lib3)) std::printf("H %lld %lld %lld\n", (long long)lib3[0], (long long)lib3[1], (long long)lib3[2]);
            else std::puts("H none");
            sv_sort(rows);
            int64_t n_assigned = 0;
            for (const SvPairCandidate& c : sv_cluster_pairs(rows, gap, percent, support, lib, flank, &n_assigned))
                std::printf("K %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)c.type,
                            (long long)c.pos, (long long)c.len, (long long)c.dv, (long long)c.dv_fwd, (long long)c.dv_rev, (long long)c.hp[0],
                            (long long)c.hp[1], (long long)c.hp[2], (long long)c.pos_min, (long long)c.pos_max, (long long)c.len_min,
                            (long long)c.len_max, (long long)c.sr, (long long)c.pr, (long long)c.end_min, (long long)c.end_max,
                            (long long)c.imprecise);
            std::printf("E %lld\n", (long long)n_assigned);
            rows.clear();
            clear_reads();
        }
    }
    std::printf("sv_pairs_check: ok, %lld reads\n", n_reads);
    return 0;
}
