"""A gVCF beside the final VCF: the variant records plus reference-confidence blocks over the rest of every chromosome.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --gvcf [--gvcf_gq_binsize 5]
    python -m hello_amd.gvcf --vcf results.output.vcf --bam illumina.bam[,pacbio.bam] --ref genome.fa --output out.g.vcf

Not in the reference; DESIGN.md section 7f defines the rules.  ``count_positions``, ``position_calls``, ``blocks_of``,
``join_blocks`` and ``block_line`` / ``block_lines`` restate them in plain NumPy / Python without a GPU; ``find_blocks`` binds
``hello_refblocks_find`` (hello_amd/csrc/refblocks.hip), which equals the restatement integer for integer; ``write_gvcf`` is the
driver pass: its own walk over the BAM(s) after scoring, one call per span of at most ``hotspots.MAX_LAUNCH_BASES`` positions,
blocks that meet at a span boundary joined on the host.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import math
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, handle_array, handle_stats, i32, i64, vp
from .bam import BamFile, Reads

ERROR_RATE = 0.001
A = -10.0 * math.log10(ERROR_RATE)           # a read base that disagrees with the genotype
B = -10.0 * math.log10(1.0 - ERROR_RATE)     # one that agrees
HET = -10.0 * math.log10(0.5)                # either, under 0/1
NO_CALL = -1                               # the band of every no-call position (HELLO_REFBLOCKS_NO_CALL)
EXCLUDED = -2
KEEP_COUNTS = 1
DEFAULT_GQ_BINSIZE = 5
FIELDS = (("start", 0, np.int64), ("end", 1, np.int64), ("band", 2, np.int32), ("min_dp", 3, np.int32), ("gq", 4, np.int32),
          ("n_ref", 5, np.int32), ("n_total", 6, np.int32))
COUNT_REF, COUNT_TOTAL = 7, 8
STAT_NAMES = ("tiles", "reads_counted", "runs", "blocks", "kernel_ms", "plan_ms", "total_ms")
NON_REF_HEADER = ('##ALT=<ID=NON_REF,Description="Represents any possible alternative allele at this location">\n'
                  '##INFO=<ID=END,Number=1,Type=Integer,Description="Last position (1-based) of the reference-confidence block">\n')
FORMAT_HEADER = dict(
    GQ='##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: QUAL rounded, at most 99">\n',
    MIN_DP='##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description="Smallest number of counted read bases at a position of the block">\n',
    PL='##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods from the pair posteriors, at most 255">\n')

Blocks = Dict[str, np.ndarray]
_log = logging.getLogger(__name__)


# ------------------------------------------------------------------------------------------------
# the rules, restated
# ------------------------------------------------------------------------------------------------
def usable(flag: int, mapq: int) -> bool:
    """``usable`` of hello_amd/csrc/cigar.h: mapped, primary, not a duplicate, a proper pair if paired, mapq > 0."""
    if flag & (0x4 | 0x100 | 0x800 | 0x400):
        return False
    if (flag & 0x1) and not (flag & 0x2):
        return False
    return mapq > 0


def counted(flag: int, mapq: int, mapq_threshold: int) -> bool:
    return usable(flag, mapq) and not (flag & 0x200) and mapq >= mapq_threshold


def _bytes_of(reference) -> np.ndarray:
    if isinstance(reference, np.ndarray):
        return reference
    return np.frombuffer(reference.encode("latin-1") if isinstance(reference, str) else bytes(reference), np.uint8)


def count_positions(reads: Sequence[Reads], reference, lo: int, hi: int, q_threshold: int = 10,
                    mapq_threshold: int = 10) -> Tuple[np.ndarray, np.ndarray]:
    """(n_ref, n_total), int32 [hi - lo], of the read sets (one per BAM) over [lo, hi)."""
    ref = _bytes_of(reference)
    n_ref, n_total = np.zeros(hi - lo, np.int32), np.zeros(hi - lo, np.int32)
    acgt = np.zeros(256, bool)
    acgt[list(b"ACGT")] = True
    for rd in reads:
        for r in range(rd.n_reads):
            if not counted(int(rd.flags[r]), int(rd.mapq[r]), mapq_threshold):
                continue
            b0, b1 = int(rd.read_offsets[r]), int(rd.read_offsets[r + 1])
            ops = [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]
            if sum(n for op, n in ops if op in (0, 1, 4, 7, 8)) > b1 - b0:
                raise ValueError(f"read {r}: its CIGAR consumes more bases than it has")
            p, i = int(rd.ref_starts[r]), 0
            for k, (op, n) in enumerate(ops):
                j0, j1 = max(lo - p, 0), min(hi - p, n)
                if op in (0, 7, 8):
                    if j1 > j0:
                        base = rd.bases[b0 + i + j0:b0 + i + j1] & 0xDF
                        ok = (rd.quals[b0 + i + j0:b0 + i + j1] >= q_threshold) & acgt[base]
                        same = ok & (base == (ref[p + j0:p + j1] & 0xDF))
                        following = [o for o, _ in ops[k + 1:] if o != 6]
                        if following and following[0] == 1 and j1 == n:       # the last base anchors an insertion
                            same[-1] = False
                        n_total[p + j0 - lo:p + j1 - lo] += ok
                        n_ref[p + j0 - lo:p + j1 - lo] += same
                    p += n
                    i += n
                elif op == 2:
                    if j1 > j0:
                        n_total[p + j0 - lo:p + j1 - lo] += 1
                    p += n
                elif op == 3:
                    p += n
                elif op in (1, 4):
                    i += n
    return n_ref, n_total


def likelihoods(n_ref, n_total) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(L00, L01, L11) in float64, in the kernel's order of operations."""
    n_ref, n_total = np.asarray(n_ref, np.int64), np.asarray(n_total, np.int64)
    nr, nt, na = n_ref.astype(np.float64), n_total.astype(np.float64), (n_total - n_ref).astype(np.float64)
    return (A * na) + (B * nr), HET * nt, (A * nr) + (B * na)


def position_calls(n_ref, n_total) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per position: called (bool), GQ (int32, 0 where not called), PL (int32 [n, 3])."""
    l00, l01, l11 = likelihoods(n_ref, n_total)
    m = np.minimum(l00, np.minimum(l01, l11))
    pl = np.stack([np.minimum(255.0, np.floor((l - m) + 0.5)) for l in (l00, l01, l11)], axis=-1).astype(np.int32)
    called = (l00 < l01) & (l00 < l11)
    gq = np.where(called, np.minimum(99, np.minimum(pl[..., 1], pl[..., 2])), 0).astype(np.int32)
    return called, gq, pl


def empty_blocks() -> Blocks:
    return {name: np.zeros(0, dtype) for name, _, dtype in FIELDS}


def blocks_of(n_ref, n_total, excluded: Sequence[Tuple[int, int]] = (), gq_binsize: int = DEFAULT_GQ_BINSIZE, lo: int = 0) -> Blocks:
    """The blocks of the positions [lo, lo + len(n_total)): maximal runs of one band outside the excluded intervals (genome
    coordinates).  Per block the smallest depth, the smallest GQ and the counters of the first position with that GQ."""
    if gq_binsize < 1:
        raise ValueError("gq_binsize: at least 1")
    n_ref, n_total = np.asarray(n_ref, np.int32), np.asarray(n_total, np.int32)
    n = n_total.shape[0]
    if n == 0:
        return empty_blocks()
    called, gq, _ = position_calls(n_ref, n_total)
    key = np.where(called, gq // gq_binsize, NO_CALL).astype(np.int64)
    for a, b in excluded:
        key[max(a - lo, 0):max(b - lo, 0)] = EXCLUDED
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    last = np.concatenate([first[1:], [n]])
    packed = np.minimum.reduceat(gq.astype(np.int64) * n + np.arange(n), first)
    at = packed % n
    keep = key[first] != EXCLUDED
    out = dict(start=lo + first, end=lo + last, band=key[first], min_dp=np.minimum.reduceat(n_total, first), gq=packed // n,
               n_ref=n_ref[at], n_total=n_total[at])
    return {name: np.asarray(out[name][keep], dtype) for name, _, dtype in FIELDS}


def join_blocks(parts: Sequence[Blocks]) -> Blocks:
    """The blocks of consecutive spans as one list: two blocks that meet at a span boundary with one band become one, with the
    smaller depth, the smaller GQ and the counters of the first position with that GQ."""
    done: List[Blocks] = []
    held: Optional[dict] = None
    for part in parts:
        if part["start"].shape[0] == 0:
            continue
        part = {k: v.copy() for k, v in part.items()}
        if held is not None:
            if held["end"] == part["start"][0] and held["band"] == part["band"][0]:
                part["start"][0] = held["start"]
                part["min_dp"][0] = min(held["min_dp"], part["min_dp"][0])
                if not part["gq"][0] < held["gq"]:
                    part["gq"][0], part["n_ref"][0], part["n_total"][0] = held["gq"], held["n_ref"], held["n_total"]
            else:
                done.append({k: np.array([v]) for k, v in held.items()})
        held = {k: v[-1] for k, v in part.items()}
        done.append({k: v[:-1] for k, v in part.items()})
    if held is not None:
        done.append({k: np.array([v]) for k, v in held.items()})
    if not done:
        return empty_blocks()
    return {name: np.concatenate([d[name] for d in done]).astype(dtype) for name, _, dtype in FIELDS}


_LINE = "%s\t%d\t.\t%s\t<NON_REF>\t.\t.\tEND=%d\tGT:GQ:MIN_DP:PL\t%s:%d:%d:%d,%d,%d"


def _base(ref_byte) -> str:
    base = (chr(ref_byte) if isinstance(ref_byte, (int, np.integer)) else str(ref_byte)).upper()
    return base if base in ("A", "C", "G", "T") else "N"


def block_line(chromosome: str, start: int, end: int, band: int, gq: int, min_dp: int, n_ref: int, n_total: int, ref_byte) -> str:
    """One block as a gVCF line (no newline).  ``ref_byte``: the reference byte (or character) at ``start``."""
    pl = position_calls([n_ref], [n_total])[2][0]
    return _LINE % (chromosome, start + 1, _base(ref_byte), end, "./." if band == NO_CALL else "0/0", gq, min_dp, pl[0], pl[1], pl[2])


def block_lines(chromosome: str, blocks: Blocks, reference) -> List[str]:
    """``block_line`` of every block, with the likelihoods of all blocks computed at once."""
    ref = _bytes_of(reference)
    pl = position_calls(blocks["n_ref"], blocks["n_total"])[2].tolist()
    bases = [_base(b) for b in ref[blocks["start"]].tolist()] if blocks["start"].shape[0] else []
    rows = zip(blocks["start"].tolist(), bases, blocks["end"].tolist(), blocks["band"].tolist(), blocks["gq"].tolist(),
               blocks["min_dp"].tolist(), pl)
    return [_LINE % (chromosome, s + 1, b, e, "./." if band == NO_CALL else "0/0", gq, dp, p[0], p[1], p[2])
            for s, b, e, band, gq, dp, p in rows]


def gvcf_header(header: str) -> str:
    """The header of the final VCF with the lines a gVCF adds, before the column line."""
    lines = header.splitlines(keepends=True)
    add = NON_REF_HEADER + "".join(text for key, text in FORMAT_HEADER.items()
                                   if not any(line.startswith("##FORMAT=<ID=%s," % key) for line in lines))
    at = next((i for i, line in enumerate(lines) if line.startswith("#CHROM")), len(lines))
    return "".join(lines[:at]) + add + "".join(lines[at:])


def excluded_intervals(records: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """(POS - 1, len(REF)) of every record of one chromosome -> sorted intervals, merged where they touch or overlap."""
    out: List[Tuple[int, int]] = []
    for a, b in sorted((p, p + n) for p, n in records):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_refblocks_find", READS + [i64, vp, i64, i64, i64, vp, vp, i64, i32, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_refblocks_array", ARRAY_GETTER),
    ("hello_refblocks_stats", STATS_GETTER),
    ("hello_refblocks_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def find_blocks(reads: Sequence[Reads], reference, lo: int, hi: int, excluded: Sequence[Tuple[int, int]] = (),
                q_threshold: int = 10, mapq_threshold: int = 10, gq_binsize: int = DEFAULT_GQ_BINSIZE, keep_counts: bool = False,
                device: int = 0):
    """One ``hello_refblocks_find`` call over already decoded read sets (one per BAM, at most two) -> (blocks, statistics,
    (n_ref, n_total) with ``keep_counts`` else None).  ``excluded``: sorted intervals that do not overlap, genome coordinates."""
    if not 1 <= len(reads) <= 2:
        raise ValueError("one or two read sets (BAM files)")
    r, source = Reads.concat(list(reads))
    ref = _bytes_of(reference)
    starts = np.array([a for a, _ in excluded], np.int64)
    stops = np.array([b for _, b in excluded], np.int64)
    lib = _lib()
    h = C.c_void_p()
    ptr = lambda a: a.ctypes.data  # noqa: E731
    check(lib.hello_refblocks_find(*r.pointers(source), int(r.n_reads), ptr(ref), int(ref.shape[0]), int(lo), int(hi), ptr(starts),
                                   ptr(stops), int(starts.shape[0]), int(q_threshold), int(mapq_threshold), int(gq_binsize),
                                   KEEP_COUNTS if keep_counts else 0, int(device), C.byref(h)))
    try:
        def array(which, dtype):
            return handle_array(lib.hello_refblocks_array, h, which, dtype)
        blocks = {name: array(which, dtype) for name, which, dtype in FIELDS}
        counts = (array(COUNT_REF, np.int32), array(COUNT_TOTAL, np.int32)) if keep_counts else None
        return blocks, handle_stats(lib.hello_refblocks_stats, h, STAT_NAMES), counts
    finally:
        lib.hello_refblocks_free(h)


# ------------------------------------------------------------------------------------------------
# the file
# ------------------------------------------------------------------------------------------------
def read_vcf(path: str):
    """-> (header text, [(chromosome, POS - 1, len(REF), the line's bytes with its newline)] in file order)."""
    header, records = [], []
    with open(path, "rb") as fh:
        for line in fh:
            if line.startswith(b"#"):
                header.append(line)
                continue
            if not line.strip():
                continue
            f = line.split(b"\t", 4)
            records.append((f[0].decode(), int(f[1]) - 1, len(f[3]), line))
    return b"".join(header).decode(), records


def chromosome_blocks(handles: Sequence[BamFile], chromosome: str, reference, excluded: Sequence[Tuple[int, int]], q_threshold: int,
                      mapq_threshold: int, gq_binsize: int, device: int = 0, restatement: bool = False,
                      max_span: Optional[int] = None, stats: Optional[dict] = None) -> Blocks:
    """The blocks of one whole chromosome: one call per span of at most ``max_span`` positions, joined at the span boundaries."""
    from .spans import adder, span_step
    ref = _bytes_of(reference)
    length, step, add = int(ref.shape[0]), span_step(max_span), adder(stats)
    parts = []
    for lo in range(0, length, step):
        hi = min(lo + step, length)
        t0 = time.perf_counter()
        sets = [h.fetch(chromosome, lo, hi) for h in handles]
        t1 = time.perf_counter()
        inside = [(a, b) for a, b in excluded if b > lo and a < hi]
        if restatement:
            n_ref, n_total = count_positions(sets, ref, lo, hi, q_threshold, mapq_threshold)
            blocks, st = blocks_of(n_ref, n_total, inside, gq_binsize, lo), {}
        else:
            blocks, st, _ = find_blocks(sets, ref, lo, hi, inside, q_threshold, mapq_threshold, gq_binsize, device=device)
        add("decode_s", t1 - t0)
        add("find_s", time.perf_counter() - t1)
        add("calls", 1)
        for k, v in st.items():
            add(k, v)
        parts.append(blocks)
    t0 = time.perf_counter()
    joined = join_blocks(parts)
    add("join_s", time.perf_counter() - t0)
    return joined


def write_gvcf(vcf_path: str, bams: Sequence[str], fasta, out_path: str, chromosomes: Optional[Sequence[str]] = None,
               q_threshold: int = 10, mapq_threshold: int = 10, gq_binsize: int = DEFAULT_GQ_BINSIZE, device: int = 0,
               restatement: bool = False, max_span: Optional[int] = None, stats: Optional[dict] = None) -> str:
    """``out_path``: the header of ``vcf_path`` with the gVCF's declarations, its records byte for byte, and the reference-confidence
    blocks of every chromosome of ``chromosomes`` (default: all of the FASTA) from 0 to its length outside the records' reference
    alleles, sorted by (chromosome name, position).  ``fasta``: a path, or {chromosome: sequence}.  ``restatement``: the blocks come
    from ``count_positions`` / ``blocks_of`` instead of the GPU (what the tests compare the GPU's file with)."""
    if not 1 <= len(bams) <= 2:
        raise ValueError("one BAM, or an Illumina and a PacBio BAM")
    if isinstance(fasta, str):
        from .call import read_fasta
        genome = read_fasta(fasta, chromosomes)
    else:
        genome = fasta
    names = list(chromosomes) if chromosomes else list(genome)
    for c in names:
        if c not in genome:
            raise ValueError(f"no sequence named {c!r} in the reference")
    header, records = read_vcf(vcf_path)
    by_chromosome: Dict[str, list] = {}
    for rec in records:
        by_chromosome.setdefault(rec[0], []).append(rec)
    handles = [BamFile(p) for p in bams]
    t_write = 0.0
    try:
        with open(out_path, "wb") as out:
            out.write(gvcf_header(header).encode("ascii"))
            for c in sorted(set(names) | set(by_chromosome)):              # the chromosome order of merge_final_vcf
                recs = by_chromosome.get(c, [])
                blocks = empty_blocks()
                if c in names:
                    ref = _bytes_of(genome[c])
                    excluded = [(a, min(b, int(ref.shape[0]))) for a, b in excluded_intervals([(p, n) for _, p, n, _ in recs])
                                if a < ref.shape[0]]
                    blocks = chromosome_blocks(handles, c, ref, excluded, q_threshold, mapq_threshold, gq_binsize, device, restatement,
                                               max_span, stats)
                t0 = time.perf_counter()
                k = 0
                lines = block_lines(c, blocks, ref) if blocks["start"].shape[0] else []
                for start, line in zip(blocks["start"].tolist(), lines):
                    while k < len(recs) and recs[k][1] < start:
                        out.write(recs[k][3])
                        k += 1
                    out.write(line.encode("ascii") + b"\n")
                for rec in recs[k:]:
                    out.write(rec[3])
                t_write += time.perf_counter() - t0
                _log.info("chromosome %s: %d records, %d reference-confidence blocks", c, len(recs), blocks["start"].shape[0])
    finally:
        for h in handles:
            h.close()
    if stats is not None:
        stats["write_s"] = stats.get("write_s", 0.0) + t_write
    return out_path


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Write a gVCF from a VCF that already exists and the BAM(s) it was called from")
    p.add_argument("--vcf", required=True, help="The VCF whose records the gVCF keeps (results.output.vcf)")
    p.add_argument("--bam", required=True, help="The BAM, or Illumina,PacBio")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--output", required=True, help="Path of the gVCF")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes to cover (default: every FASTA record)")
    p.add_argument("--q_threshold", type=int, default=10, help="Base quality threshold")
    p.add_argument("--mapq_threshold", type=int, default=10, help="Mapping quality threshold")
    p.add_argument("--gvcf_gq_binsize", type=int, default=DEFAULT_GQ_BINSIZE, help="Width of a GQ band")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> str:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    if args.gvcf_gq_binsize < 1:
        raise SystemExit("--gvcf_gq_binsize: at least 1")
    bams = args.bam.split(",")
    if len(bams) > 2:
        raise SystemExit("--bam takes one or two files")
    return write_gvcf(args.vcf, bams, args.ref, args.output, args.chromosomes.split(",") if args.chromosomes else None,
                      args.q_threshold, args.mapq_threshold, args.gvcf_gq_binsize, args.device)


if __name__ == "__main__":
    main(sys.argv[1:])
