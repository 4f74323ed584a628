// The rules of the split alignments -- parse_sa_entry, sv_junction and sv_split_read of hello_amd/csrc/sv_split.h, and the clusters
// of hello_amd/csrc/sv.h with their SR column -- as a stand-alone host program: built by tests/test_sv_split.py with
// -fsanitize=address,undefined and run directly on a file of reads and tags the test writes (the hand cases, the stress and the
// fuzz of tests/sv_split_cases.py).  It prints what it finds; the test compares that with the restatement of hello_amd/sv.py.
//
// Input, line by line:  P length own min_size flank mapq_threshold cluster_gap len_ratio_percent min_support / C contig name /
// F reference text / R ref_start flag mapq hp ordinal CIGAR tag-in-hex / E (the end of one block: prints its clusters).
// Output: per R one line "S status junctions dropped small unplaced" and a line "G" with the eight columns per row; per E a line
// "K" with the fourteen columns per cluster and a line "E".  Every tag is copied into an array of exactly its size first, so that a
// byte index that leaves it is caught.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../hello_amd/csrc/sv_split.h"

using namespace hello;

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: sv_split_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) return 2;
    long long length = 0, own = 0, min_size = 1, flank = 1, mapq_threshold = 0, gap = 0, percent = 100, support = 1;
    std::vector<uint64_t> hashes;
    std::vector<uint8_t> ref;
    std::vector<SvSig> rows;
    std::string line;
    long long n_reads = 0;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        char kind = 0;
        f >> kind;
        if (kind == 'P') {
            f >> length >> own >> min_size >> flank >> mapq_threshold >> gap >> percent >> support;
            hashes.clear();
            rows.clear();
        } else if (kind == 'C') {
            std::string name;
            f >> name;
            hashes.push_back(sv_name_hash(name));
        } else if (kind == 'F') {
            std::string text;
            f >> text;
            ref.assign(text.begin(), text.end());
            if ((long long)ref.size() != length) return 3;
        } else if (kind == 'R') {
            long long s = 0, flag = 0, mapq = 0, hp = 0, ordinal = 0;
            std::string cigar, hex;
            f >> s >> flag >> mapq >> hp >> ordinal >> cigar >> hex;
            const size_t n = hex.size() / 2;
            std::unique_ptr<uint8_t[]> tag(new uint8_t[n]);                 // exactly n bytes
            for (size_t i = 0; i < n; ++i) tag[i] = (uint8_t)std::strtol(hex.substr(2 * i, 2).c_str(), nullptr, 16);
            std::unique_ptr<uint8_t[]> text(new uint8_t[cigar.size()]);
            for (size_t i = 0; i < cigar.size(); ++i) text[i] = (uint8_t)cigar[i];
            SvSegment primary{};
            int64_t i = 0, r = 0;
            primary.ok = sa_cigar(text.get(), i, (int64_t)cigar.size(), primary, r) && i == (int64_t)cigar.size();
            primary.s = s;
            primary.e = s + r;
            primary.tid = (int32_t)own;
            primary.mapq = (int32_t)mapq;
            primary.strand = (flag & 0x10) ? 1 : 0;
            sv_orient(primary);
            const SvSplitRead got = sv_split_read(primary, tag.get(), (int64_t)n, hashes.data(), (int64_t)hashes.size(), (int32_t)own, ref.data(),
                                                  length, min_size, flank, (int32_t)mapq_threshold, ordinal, (uint8_t)primary.strand, (uint8_t)hp);
            std::printf("S %d %lld %lld %lld %lld\n", got.status, (long long)got.junctions, (long long)got.dropped, (long long)got.small,
                        (long long)got.unplaced);
            for (const SvSig& g : got.rows) {
                std::printf("G %d %lld %d %d %lld %lld %d %d\n", g.type, (long long)g.pos, g.len, g.shift, (long long)g.ordinal,
                            (long long)g.op_index, g.strand, g.hp);
                rows.push_back(g);
            }
            ++n_reads;
        } else if (kind == 'E') {
            sv_sort(rows);
            for (const SvCandidate& c : sv_cluster(rows, gap, percent, support))
                std::printf("K %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)c.type, (long long)c.pos,
                            (long long)c.len, (long long)c.dv, (long long)c.dv_fwd, (long long)c.dv_rev, (long long)c.hp[0], (long long)c.hp[1],
                            (long long)c.hp[2], (long long)c.pos_min, (long long)c.pos_max, (long long)c.len_min, (long long)c.len_max,
                            (long long)c.sr);
            std::puts("E");
            rows.clear();
        }
    }
    std::printf("sv_split_check: ok, %lld reads\n", n_reads);
    return 0;
}
