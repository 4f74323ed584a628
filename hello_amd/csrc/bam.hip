// BAM reader (include/hello_mi355x.h: hello_bam_*), host only.  Stands in for the pysam AlignmentFile.fetch the reference's
// read containers run per chunk (python/PileupContainerLite.py:526-570 through python/PileupDataTools.py:130-160).
//
// BGZF blocks are inflated with zlib by up to 16 host threads in batches; the decompressed stream is parsed into flat arrays in
// the layout hello_engine_featurize and hello_hotspots_find take.  A region is located with the `.bai` linear index when one
// exists (the smallest virtual offset of a record overlapping the region's first 16 kbp window), otherwise the whole file is
// scanned.  Records overlap [start, stop) as htslib's fetch decides it: pos < stop and end > start, where a record without
// reference-consuming operations (or an unmapped one) ends at pos + 1 (bam_endpos).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <zlib.h>

#include "../../include/hello_mi355x.h"
#include "mods.h"

namespace hello {
int set_last_error(int code, const char* fmt, ...);      // engine.hip
int exception_status(const char* where) noexcept;         // engine.hip
}  // namespace hello

struct hello_bam {
    std::string path;
    FILE* fh = nullptr;
    int threads = 1;
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    uint64_t first_record = 0;          // virtual offset of the first alignment record
    ~hello_bam() { if (fh) fclose(fh); }
};

struct hello_bam_reads {
    std::vector<uint8_t> bases, quals;
    std::vector<int64_t> read_off{0}, cigar_off{0}, ref_start, ref_end;
    std::vector<uint32_t> cigars;
    std::vector<uint8_t> mapq, strand, hp;
    std::vector<uint16_t> flag;
    std::vector<uint64_t> name_hash;
    std::vector<int32_t> mod_deltas;    // hello_bam_fetch_mods alone fills these five
    std::vector<uint8_t> mod_probs, mod_mode, mod_state;
    std::vector<int64_t> mod_off{0};
    std::vector<uint8_t> sa_bytes;      // hello_bam_fetch_sa alone fills these two
    std::vector<int64_t> sa_off;
    bool with_sa = false;               // made by hello_bam_fetch_sa or hello_bam_fetch_pairs: the two SA selectors exist for them alone
    std::vector<int32_t> mate_tid, tlen;        // hello_bam_fetch_pairs alone fills these three
    std::vector<int64_t> mate_pos;
    bool with_pairs = false;
    int32_t used_index = 0;
    int64_t blocks = 0;
};

namespace {

using hello::set_last_error;

struct BamError {
    int code;
    std::string msg;
};
[[noreturn]] void raise(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw BamError{code, buf};
}

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

// The decompressed byte stream of a BGZF file from a virtual offset on: batches of blocks are read, then inflated in parallel.
struct Stream {
    FILE* fh;
    int threads;
    const std::string& path;
    int64_t coff = 0;          // file offset of the next block to read
    bool at_end = false;
    std::vector<uint8_t> buf;
    size_t pos = 0;
    uint64_t consumed = 0;     // bytes dropped from the front of `buf`
    int64_t blocks = 0;

    Stream(FILE* f, int t, const std::string& p) : fh(f), threads(t), path(p) {}

    void seek(uint64_t voff) {
        coff = (int64_t)(voff >> 16);
        buf.clear();
        pos = 0;
        at_end = false;
        fill(1);
        if ((voff & 0xffff) > buf.size()) raise(HELLO_ERR_SHAPE, "%s: virtual offset points past its block", path.c_str());
        pos = voff & 0xffff;
    }

    // read up to `want` blocks; false at the end of the file
    bool fill(int want) {
        if (at_end) return false;
        std::vector<std::vector<uint8_t>> comp;
        std::vector<uint32_t> isize;
        if (fseeko(fh, coff, SEEK_SET) != 0) raise(HELLO_ERR_ARG, "%s: seek failed", path.c_str());
        for (int b = 0; b < want; ++b) {
            uint8_t h[18];
            size_t got = fread(h, 1, 18, fh);
            if (got == 0) { at_end = true; break; }
            if (got < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4))
                raise(HELLO_ERR_ARG, "%s: not a BGZF file (BAM is BGZF-compressed) at offset %lld", path.c_str(), (long long)coff);
            const int xlen = rd16(h + 10);
            if (xlen < 6 || h[12] != 'B' || h[13] != 'C' || rd16(h + 14) != 2)
                raise(HELLO_ERR_ARG, "%s: gzip block without the BGZF 'BC' field at offset %lld", path.c_str(), (long long)coff);
            const int bsize = rd16(h + 16) + 1;
            if (bsize < 18 + 8) raise(HELLO_ERR_ARG, "%s: truncated BGZF block at offset %lld", path.c_str(), (long long)coff);
            std::vector<uint8_t> block(bsize);
            memcpy(block.data(), h, 18);
            if (fread(block.data() + 18, 1, bsize - 18, fh) != (size_t)(bsize - 18))
                raise(HELLO_ERR_ARG, "%s: truncated BGZF block at offset %lld", path.c_str(), (long long)coff);
            isize.push_back(rd32(block.data() + bsize - 4));
            comp.push_back(std::move(block));
            coff += bsize;
        }
        if (comp.empty()) return false;
        if (pos > 0) { buf.erase(buf.begin(), buf.begin() + pos); consumed += pos; pos = 0; }
        const size_t base = buf.size();
        std::vector<size_t> out_off(comp.size() + 1, base);
        for (size_t i = 0; i < comp.size(); ++i) out_off[i + 1] = out_off[i] + isize[i];
        buf.resize(out_off.back());
        std::vector<int> status(comp.size(), 0);
        auto inflate_range = [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                const auto& c = comp[i];
                const int xlen = rd16(c.data() + 10);
                z_stream z{};
                if (inflateInit2(&z, -15) != Z_OK) { status[i] = -1; continue; }
                z.next_in = const_cast<uint8_t*>(c.data() + 12 + xlen);
                z.avail_in = (uInt)(c.size() - 12 - xlen - 8);
                z.next_out = buf.data() + out_off[i];
                z.avail_out = isize[i];
                const int rc = inflate(&z, Z_FINISH);
                if (rc != Z_STREAM_END || z.total_out != isize[i]) status[i] = -1;
                else if (crc32(0L, buf.data() + out_off[i], isize[i]) != rd32(c.data() + c.size() - 8)) status[i] = -2;
                inflateEnd(&z);
            }
        };
        const int nt = std::max(1, std::min<int>(threads, (int)comp.size()));
        if (nt == 1) {
            inflate_range(0, comp.size());
        } else {
            std::vector<std::thread> pool;
            const size_t per = (comp.size() + nt - 1) / nt;
            for (int t = 0; t < nt; ++t) {
                const size_t lo = t * per, hi = std::min(comp.size(), lo + per);
                if (lo < hi) pool.emplace_back(inflate_range, lo, hi);
            }
            for (auto& th : pool) th.join();
        }
        for (size_t i = 0; i < comp.size(); ++i)
            if (status[i]) raise(HELLO_ERR_ARG, "%s: corrupt BGZF block (%s)", path.c_str(), status[i] == -2 ? "CRC mismatch" : "inflate failed");
        blocks += (int64_t)comp.size();
        return true;
    }

    bool ensure(size_t n) {
        while (buf.size() - pos < n)
            if (!fill(std::max(16, 8 * threads))) return false;
        return true;
    }
    const uint8_t* take(size_t n, const char* what) {
        if (!ensure(n)) raise(HELLO_ERR_ARG, "%s: file ends inside %s", path.c_str(), what);
        const uint8_t* p = buf.data() + pos;
        pos += n;
        return p;
    }
};

void check_magic(FILE* fh, const std::string& path) {
    uint8_t m[4] = {0, 0, 0, 0};
    const size_t got = fread(m, 1, 4, fh);
    if (got == 4 && memcmp(m, "CRAM", 4) == 0)
        raise(HELLO_ERR_ARG, "%s is a CRAM file: only BAM input is supported (convert it with `samtools view -b`)", path.c_str());
    if (got < 2 || m[0] != 31 || m[1] != 139) raise(HELLO_ERR_ARG, "%s is not a BAM file (no BGZF header)", path.c_str());
    fseeko(fh, 0, SEEK_SET);
}

uint64_t fnv1a(const uint8_t* s, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= s[i]; h *= 1099511628211ull; }
    return h;
}

// .bai linear index: smallest virtual offset of a record overlapping [start, ...) on `tid`; 0 = nothing there; UINT64_MAX = no index
uint64_t index_offset(const std::string& bam_path, int tid, int64_t start, bool* empty) {
    std::string cand[2] = {bam_path + ".bai", bam_path};
    if (cand[1].size() > 4 && cand[1].compare(cand[1].size() - 4, 4, ".bam") == 0) cand[1].replace(cand[1].size() - 4, 4, ".bai");
    else cand[1].clear();
    FILE* f = nullptr;
    for (auto& c : cand)
        if (!c.empty() && (f = fopen(c.c_str(), "rb"))) break;
    if (!f) return UINT64_MAX;
    std::vector<uint8_t> d;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) d.insert(d.end(), tmp, tmp + n);
    fclose(f);
    size_t p = 0;
    auto need = [&](size_t k) { if (p + k > d.size()) raise(HELLO_ERR_ARG, "%s: truncated .bai index", bam_path.c_str()); };
    need(8);
    if (memcmp(d.data(), "BAI\1", 4) != 0) raise(HELLO_ERR_ARG, "%s: its .bai index has no BAI magic", bam_path.c_str());
    const int32_t n_ref = (int32_t)rd32(d.data() + 4);
    p = 8;
    if (tid >= n_ref) raise(HELLO_ERR_ARG, "%s: its .bai index holds %d references, the header more", bam_path.c_str(), n_ref);
    for (int r = 0; r <= tid; ++r) {
        need(4);
        const int32_t n_bin = (int32_t)rd32(d.data() + p);
        p += 4;
        uint64_t min_beg = UINT64_MAX;
        for (int b = 0; b < n_bin; ++b) {
            need(8);
            const uint32_t bin = rd32(d.data() + p);
            const int32_t n_chunk = (int32_t)rd32(d.data() + p + 4);
            p += 8;
            need((size_t)n_chunk * 16);
            if (bin != 37450)                                         // the pseudo-bin holds statistics, not chunks
                for (int c = 0; c < n_chunk; ++c) min_beg = std::min(min_beg, rd64(d.data() + p + 16 * c));
            p += (size_t)n_chunk * 16;
        }
        need(4);
        const int32_t n_intv = (int32_t)rd32(d.data() + p);
        p += 4;
        need((size_t)n_intv * 8);
        if (r == tid) {
            *empty = false;
            if (n_bin == 0 || min_beg == UINT64_MAX) { *empty = true; return 0; }
            const int64_t k = start >> 14;
            if (k >= n_intv) { *empty = true; return 0; }             // no record reaches this far
            uint64_t off = 0;
            for (int64_t j = k; j >= 0 && off == 0; --j) off = rd64(d.data() + p + 8 * j);
            return off ? std::max(off, min_beg) : min_beg;
        }
        p += (size_t)n_intv * 8;
    }
    return UINT64_MAX;
}

constexpr char kSeqCodes[] = "=ACMGRSVTWYHKDBN";

// The CG:B,I tag of a record whose CIGAR has more than 65535 operations (SAM specification 4.2.2: the CIGAR field then holds the
// placeholder <l_seq>S<reference length>N).  Returns the tag's operation array and count, or nullptr when there is none.
const uint8_t* find_cg_tag(const uint8_t* aux, const uint8_t* end, uint32_t* count, const std::string& path) {
    auto bad = [&]() { raise(HELLO_ERR_ARG, "%s: malformed auxiliary field", path.c_str()); };
    auto scalar = [](uint8_t t) -> int {
        switch (t) {
            case 'A': case 'c': case 'C': return 1;
            case 's': case 'S': return 2;
            case 'i': case 'I': case 'f': return 4;
            default: return 0;
        }
    };
    while (aux < end) {
        if (end - aux < 3) bad();
        const uint8_t t0 = aux[0], t1 = aux[1], type = aux[2];
        aux += 3;
        if (type == 'Z' || type == 'H') {
            const uint8_t* z = (const uint8_t*)memchr(aux, 0, (size_t)(end - aux));
            if (!z) bad();
            aux = z + 1;
        } else if (type == 'B') {
            if (end - aux < 5) bad();
            const uint8_t sub = aux[0];
            const uint32_t n = rd32(aux + 1);
            const int w = scalar(sub);
            if (!w || sub == 'A' || (uint64_t)n * w > (uint64_t)(end - aux - 5)) bad();
            if (t0 == 'C' && t1 == 'G') {
                if (sub != 'I') raise(HELLO_ERR_ARG, "%s: CG tag of type B,%c (B,I expected)", path.c_str(), sub);
                *count = n;
                return aux + 5;
            }
            aux += 5 + (size_t)n * w;
        } else {
            const int w = scalar(type);
            if (!w || end - aux < w) bad();
            aux += w;
        }
    }
    return nullptr;
}

// The HP tag (haplotype of a phased read) as an integer of any BAM integer type; 0 when the record has none, when its value does
// not fit a byte, or when the auxiliary fields cannot be walked (they are nobody else's concern: no error).
uint8_t find_hp_tag(const uint8_t* aux, const uint8_t* end) {
    auto scalar = [](uint8_t t) -> int {
        switch (t) {
            case 'A': case 'c': case 'C': return 1;
            case 's': case 'S': return 2;
            case 'i': case 'I': case 'f': return 4;
            default: return 0;
        }
    };
    while (end - aux >= 3) {
        const uint8_t t0 = aux[0], t1 = aux[1], type = aux[2];
        aux += 3;
        if (type == 'Z' || type == 'H') {
            const uint8_t* z = (const uint8_t*)memchr(aux, 0, (size_t)(end - aux));
            if (!z) return 0;
            aux = z + 1;
        } else if (type == 'B') {
            if (end - aux < 5) return 0;
            const int w = scalar(aux[0]);
            const uint32_t n = rd32(aux + 1);
            if (!w || (uint64_t)n * w > (uint64_t)(end - aux - 5)) return 0;
            aux += 5 + (size_t)n * w;
        } else {
            const int w = scalar(type);
            if (!w || end - aux < w) return 0;
            if (t0 == 'H' && t1 == 'P') {
                int64_t v;
                switch (type) {
                    case 'c': v = (int8_t)aux[0]; break;
                    case 'C': v = aux[0]; break;
                    case 's': v = (int16_t)rd16(aux); break;
                    case 'S': v = rd16(aux); break;
                    case 'i': v = (int32_t)rd32(aux); break;
                    case 'I': v = rd32(aux); break;
                    default: return 0;
                }
                return (v >= 0 && v <= 255) ? (uint8_t)v : 0;
            }
            aux += w;
        }
    }
    return 0;
}

// The text of the first SA field among a record's auxiliary fields [aux, end), without its NUL: [*text, *text + n).  n = 0 where
// there is none, where it is not of type Z, or where the fields before it cannot be walked (as for HP).
size_t find_sa_tag(const uint8_t* aux, const uint8_t* end, const uint8_t** text) {
    auto scalar = [](uint8_t t) -> int {
        switch (t) {
            case 'A': case 'c': case 'C': return 1;
            case 's': case 'S': return 2;
            case 'i': case 'I': case 'f': return 4;
            default: return 0;
        }
    };
    while (end - aux >= 3) {
        const bool is_sa = aux[0] == 'S' && aux[1] == 'A';
        const uint8_t type = aux[2];
        aux += 3;
        if (type == 'Z' || type == 'H') {
            const uint8_t* z = (const uint8_t*)memchr(aux, 0, (size_t)(end - aux));
            if (!z) break;
            if (is_sa) { *text = aux; return type == 'Z' ? (size_t)(z - aux) : 0; }
            aux = z + 1;
        } else if (type == 'B') {
            if (end - aux < 5) break;
            const int w = scalar(aux[0]);
            const uint32_t n = rd32(aux + 1);
            if (is_sa || !w || (uint64_t)n * w > (uint64_t)(end - aux - 5)) break;
            aux += 5 + (size_t)n * w;
        } else {
            const int w = scalar(type);
            if (is_sa || !w || end - aux < w) break;
            aux += w;
        }
    }
    return 0;
}

enum FetchKind { kFetchPlain = 0, kFetchMods = 1, kFetchSa = 2, kFetchPairs = 3 };

// append one record (the bytes after its block_size field) to the flat arrays
void decode(hello_bam_reads* r, const uint8_t* b, int32_t block_size, const std::string& path, FetchKind kind = kFetchPlain) {
    const bool mods = kind == kFetchMods;
    const int32_t pos = (int32_t)rd32(b + 4);
    const int l_name = b[8], mapq = b[9];
    const int n_cigar = rd16(b + 12), flag = rd16(b + 14);
    const int32_t l_seq = (int32_t)rd32(b + 16);
    const size_t need = 32 + (size_t)l_name + 4 * (size_t)n_cigar + (size_t)((l_seq + 1) / 2) + (size_t)l_seq;
    if (l_seq < 0 || need > (size_t)block_size) raise(HELLO_ERR_ARG, "%s: malformed alignment record", path.c_str());
    const uint8_t* name = b + 32;
    const uint8_t* cig = name + l_name;
    const uint8_t* seq = cig + 4 * n_cigar;
    const uint8_t* qual = seq + (l_seq + 1) / 2;
    if (l_seq > 0 && qual[0] == 0xFF)
        raise(HELLO_ERR_ARG, "%s: read '%.*s' has no stored base qualities (QUAL '*'); hotspot detection needs them", path.c_str(),
              std::max(0, l_name - 1), (const char*)name);
    // a CIGAR of more than 65535 operations lives in the CG tag behind a <l_seq>S<rlen>N placeholder
    uint32_t n_ops = (uint32_t)n_cigar;
    if (n_cigar == 2 && (rd32(cig) & 15) == 4 && (rd32(cig) >> 4) == (uint32_t)l_seq && (rd32(cig + 4) & 15) == 3) {
        uint32_t n = 0;
        const uint8_t* cg = find_cg_tag(b + need, b + block_size, &n, path);
        if (cg) { cig = cg; n_ops = n; }
    }
    int64_t rlen = 0;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const uint32_t c = rd32(cig + 4 * i);
        r->cigars.push_back(c);
        const int op = c & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;
    }
    if ((flag & 4) || rlen == 0) rlen = 1;
    r->cigar_off.push_back((int64_t)r->cigars.size());
    for (int32_t i = 0; i < l_seq; ++i) {
        r->bases.push_back((uint8_t)kSeqCodes[(seq[i >> 1] >> ((~i & 1) << 2)) & 15]);
        r->quals.push_back(qual[i]);
    }
    r->read_off.push_back((int64_t)r->bases.size());
    r->ref_start.push_back(pos);
    r->ref_end.push_back(pos + rlen);
    r->mapq.push_back((uint8_t)mapq);
    r->flag.push_back((uint16_t)flag);
    r->strand.push_back((flag & 16) ? 1 : 0);
    r->name_hash.push_back(fnv1a(name, l_name > 0 ? (size_t)l_name - 1 : 0));
    r->hp.push_back(find_hp_tag(b + need, b + block_size));
    if (mods) {                                                      // MM / ML (mods.h): the 5mC calls of the record
        hello::ModsOfRead m;
        hello::find_mods(b + need, b + block_size, m);
        r->mod_deltas.insert(r->mod_deltas.end(), m.deltas.begin(), m.deltas.end());
        r->mod_probs.insert(r->mod_probs.end(), m.probs.begin(), m.probs.end());
        r->mod_off.push_back((int64_t)r->mod_deltas.size());
        r->mod_mode.push_back(m.mode);
        r->mod_state.push_back(m.state);
    }
    if (kind == kFetchPairs) {                                       // next_refID, next_pos, tlen of the fixed core, as they stand
        r->mate_tid.push_back((int32_t)rd32(b + 20));
        r->mate_pos.push_back((int64_t)(int32_t)rd32(b + 24));
        r->tlen.push_back((int32_t)rd32(b + 28));
    }
    if (kind == kFetchSa || kind == kFetchPairs) {
        const uint8_t* text = nullptr;
        const size_t n = find_sa_tag(b + need, b + block_size, &text);
        if (n) r->sa_bytes.insert(r->sa_bytes.end(), text, text + n);
        r->sa_off.push_back((int64_t)r->sa_bytes.size());
    }
}

}  // namespace

extern "C" {

int hello_bam_open(const char* path, int32_t n_threads, hello_bam** out) try {
    if (!path || !out) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    auto* bam = new hello_bam();
    std::unique_ptr<hello_bam> own(bam);
    bam->path = path;
    bam->threads = std::max(1, std::min(16, n_threads <= 0 ? 16 : (int)n_threads));
    bam->fh = fopen(path, "rb");
    if (!bam->fh) return set_last_error(HELLO_ERR_ARG, "%s: cannot open", path);
    check_magic(bam->fh, bam->path);
    Stream s(bam->fh, 1, bam->path);
    s.seek(0);
    const uint8_t* m = s.take(4, "the BAM header");
    if (memcmp(m, "BAM\1", 4) != 0) raise(HELLO_ERR_ARG, "%s: BGZF file without the BAM magic", path);
    const int32_t l_text = (int32_t)rd32(s.take(4, "the BAM header"));
    if (l_text < 0) raise(HELLO_ERR_ARG, "%s: malformed BAM header", path);
    s.take((size_t)l_text, "the BAM header text");
    const int32_t n_ref = (int32_t)rd32(s.take(4, "the BAM header"));
    if (n_ref < 0) raise(HELLO_ERR_ARG, "%s: malformed BAM header", path);
    for (int32_t i = 0; i < n_ref; ++i) {
        const int32_t l_name = (int32_t)rd32(s.take(4, "the reference list"));
        if (l_name < 1) raise(HELLO_ERR_ARG, "%s: malformed reference name", path);
        const uint8_t* nm = s.take((size_t)l_name, "the reference list");
        bam->names.emplace_back((const char*)nm, strnlen((const char*)nm, (size_t)l_name));
        bam->lengths.push_back((int64_t)rd32(s.take(4, "the reference list")));
    }
    // virtual offset of the first record: walk the block sizes (ISIZE, the last 4 bytes of a block) up to the header's end
    {
        uint64_t left = s.consumed + s.pos;
        int64_t off = 0;
        while (true) {
            uint8_t h[18], isz[4];
            if (fseeko(bam->fh, off, SEEK_SET) != 0 || fread(h, 1, 18, bam->fh) != 18) raise(HELLO_ERR_ARG, "%s: file ends inside the BAM header", path);
            const int64_t bsize = rd16(h + 16) + 1;
            if (fseeko(bam->fh, off + bsize - 4, SEEK_SET) != 0 || fread(isz, 1, 4, bam->fh) != 4) raise(HELLO_ERR_ARG, "%s: truncated BGZF block", path);
            const uint64_t isize = rd32(isz);
            if (left < isize) { bam->first_record = ((uint64_t)off << 16) | left; break; }
            left -= isize;
            off += bsize;
            if (left == 0) { bam->first_record = (uint64_t)off << 16; break; }
        }
    }
    *out = own.release();
    return HELLO_OK;
} catch (const BamError& e) {
    return set_last_error(e.code, "%s", e.msg.c_str());
} catch (...) {
    return hello::exception_status("hello_bam_open");
}

int hello_bam_n_references(const hello_bam* bam) {
    if (!bam) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    return (int)bam->names.size();
}

int hello_bam_reference(const hello_bam* bam, int32_t i, const char** name, int64_t* length) {
    if (!bam || !name || !length) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (i < 0 || i >= (int32_t)bam->names.size()) return set_last_error(HELLO_ERR_ARG, "reference %d of %zu", i, bam->names.size());
    *name = bam->names[i].c_str();
    *length = bam->lengths[i];
    return HELLO_OK;
}

static int fetch_records(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index, FetchKind kind,
                         hello_bam_reads** out, const char* entry) try {
    if (!bam || !chromosome || !out) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    *out = nullptr;
    if (start < 0 || stop < start) return set_last_error(HELLO_ERR_ARG, "region [%lld, %lld) is not a region", (long long)start, (long long)stop);
    int tid = -1;
    for (size_t i = 0; i < bam->names.size(); ++i)
        if (bam->names[i] == chromosome) { tid = (int)i; break; }
    if (tid < 0) return set_last_error(HELLO_ERR_ARG, "%s: no reference named '%s' in its header", bam->path.c_str(), chromosome);
    auto* r = new hello_bam_reads();
    std::unique_ptr<hello_bam_reads> own(r);
    if (kind == kFetchSa || kind == kFetchPairs) {
        r->with_sa = true;
        r->sa_off.push_back(0);
    }
    r->with_pairs = kind == kFetchPairs;
    Stream s(bam->fh, bam->threads, bam->path);
    bool empty = false;
    uint64_t voff = use_index == 0 ? UINT64_MAX : index_offset(bam->path, tid, start, &empty);
    if (use_index > 0 && voff == UINT64_MAX)
        return set_last_error(HELLO_ERR_ARG, "%s: no .bai index next to it", bam->path.c_str());
    const bool indexed = voff != UINT64_MAX;
    r->used_index = indexed ? 1 : 0;
    if (!(indexed && empty) && start < stop) {
        s.seek(indexed ? voff : bam->first_record);
        while (s.ensure(4)) {
            const int32_t block_size = (int32_t)rd32(s.take(4, "a record"));
            if (block_size < 32) raise(HELLO_ERR_ARG, "%s: malformed alignment record", bam->path.c_str());
            const uint8_t* b = s.take((size_t)block_size, "a record");
            const int32_t ref_id = (int32_t)rd32(b), pos = (int32_t)rd32(b + 4);
            if (indexed && (ref_id != tid || pos >= stop)) break;     // an indexed file is coordinate-sorted
            if (ref_id != tid || pos >= stop) continue;
            // end of the record (bam_endpos) for the overlap test
            const int n_cigar = rd16(b + 12), flag = rd16(b + 14), l_name = b[8];
            if ((size_t)32 + l_name + 4 * (size_t)n_cigar > (size_t)block_size) raise(HELLO_ERR_ARG, "%s: malformed alignment record", bam->path.c_str());
            int64_t rlen = 0;
            for (int i = 0; i < n_cigar; ++i) {
                const uint32_t c = rd32(b + 32 + l_name + 4 * i);
                const int op = c & 15;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;
            }
            if ((flag & 4) || rlen == 0) rlen = 1;
            if (pos + rlen <= start) continue;
            decode(r, b, block_size, bam->path, kind);
        }
    }
    r->blocks = s.blocks;
    *out = own.release();
    return HELLO_OK;
} catch (const BamError& e) {
    return set_last_error(e.code, "%s", e.msg.c_str());
} catch (...) {
    return hello::exception_status(entry);
}

int hello_bam_fetch(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index, hello_bam_reads** out) {
    return fetch_records(bam, chromosome, start, stop, use_index, kFetchPlain, out, "hello_bam_fetch");
}

int hello_bam_fetch_mods(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index,
                         hello_bam_reads** out) {
    return fetch_records(bam, chromosome, start, stop, use_index, kFetchMods, out, "hello_bam_fetch_mods");
}

int hello_bam_fetch_sa(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index, hello_bam_reads** out) {
    return fetch_records(bam, chromosome, start, stop, use_index, kFetchSa, out, "hello_bam_fetch_sa");
}

int hello_bam_fetch_pairs(hello_bam* bam, const char* chromosome, int64_t start, int64_t stop, int32_t use_index, hello_bam_reads** out) {
    return fetch_records(bam, chromosome, start, stop, use_index, kFetchPairs, out, "hello_bam_fetch_pairs");
}

int hello_bam_reads_info(const hello_bam_reads* reads, int64_t* n_reads, int32_t* used_index, int64_t* n_blocks) {
    if (!reads) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    if (n_reads) *n_reads = (int64_t)reads->ref_start.size();
    if (used_index) *used_index = reads->used_index;
    if (n_blocks) *n_blocks = reads->blocks;
    return HELLO_OK;
}

int hello_bam_reads_array(const hello_bam_reads* r, int32_t which, const void** data, int64_t* count) {
    if (!r || !data || !count) return set_last_error(HELLO_ERR_ARG, "NULL pointer");
    switch (which) {
        case HELLO_BAM_BASES: *data = r->bases.data(); *count = (int64_t)r->bases.size(); break;
        case HELLO_BAM_QUALS: *data = r->quals.data(); *count = (int64_t)r->quals.size(); break;
        case HELLO_BAM_READ_OFFSETS: *data = r->read_off.data(); *count = (int64_t)r->read_off.size(); break;
        case HELLO_BAM_CIGARS: *data = r->cigars.data(); *count = (int64_t)r->cigars.size(); break;
        case HELLO_BAM_CIGAR_OFFSETS: *data = r->cigar_off.data(); *count = (int64_t)r->cigar_off.size(); break;
        case HELLO_BAM_REF_STARTS: *data = r->ref_start.data(); *count = (int64_t)r->ref_start.size(); break;
        case HELLO_BAM_REF_ENDS: *data = r->ref_end.data(); *count = (int64_t)r->ref_end.size(); break;
        case HELLO_BAM_MAPQ: *data = r->mapq.data(); *count = (int64_t)r->mapq.size(); break;
        case HELLO_BAM_FLAGS: *data = r->flag.data(); *count = (int64_t)r->flag.size(); break;
        case HELLO_BAM_NAME_HASH: *data = r->name_hash.data(); *count = (int64_t)r->name_hash.size(); break;
        case HELLO_BAM_STRAND: *data = r->strand.data(); *count = (int64_t)r->strand.size(); break;
        case HELLO_BAM_HP: *data = r->hp.data(); *count = (int64_t)r->hp.size(); break;
        case HELLO_BAM_MOD_DELTAS: *data = r->mod_deltas.data(); *count = (int64_t)r->mod_deltas.size(); break;
        case HELLO_BAM_MOD_PROBS: *data = r->mod_probs.data(); *count = (int64_t)r->mod_probs.size(); break;
        case HELLO_BAM_MOD_OFFSETS: *data = r->mod_off.data(); *count = (int64_t)r->mod_off.size(); break;
        case HELLO_BAM_MOD_MODE: *data = r->mod_mode.data(); *count = (int64_t)r->mod_mode.size(); break;
        case HELLO_BAM_MOD_STATE: *data = r->mod_state.data(); *count = (int64_t)r->mod_state.size(); break;
        case HELLO_BAM_SA_BYTES:
        case HELLO_BAM_SA_OFFSETS:
            if (!r->with_sa) return set_last_error(HELLO_ERR_ARG, "no read array %d: hello_bam_fetch_sa alone fills it (and hello_bam_fetch_pairs)", which);
            if (which == HELLO_BAM_SA_BYTES) { *data = r->sa_bytes.data(); *count = (int64_t)r->sa_bytes.size(); }
            else { *data = r->sa_off.data(); *count = (int64_t)r->sa_off.size(); }
            break;
        case HELLO_BAM_MATE_TID:
        case HELLO_BAM_MATE_POS:
        case HELLO_BAM_TLEN:
            if (!r->with_pairs) return set_last_error(HELLO_ERR_ARG, "no read array %d: hello_bam_fetch_pairs alone fills it", which);
            if (which == HELLO_BAM_MATE_TID) { *data = r->mate_tid.data(); *count = (int64_t)r->mate_tid.size(); }
            else if (which == HELLO_BAM_MATE_POS) { *data = r->mate_pos.data(); *count = (int64_t)r->mate_pos.size(); }
            else { *data = r->tlen.data(); *count = (int64_t)r->tlen.size(); }
            break;
        default: return set_last_error(HELLO_ERR_ARG, "no read array %d", which);
    }
    return HELLO_OK;
}

void hello_bam_reads_free(hello_bam_reads* reads) { delete reads; }
void hello_bam_close(hello_bam* bam) { delete bam; }

}  // extern "C"
