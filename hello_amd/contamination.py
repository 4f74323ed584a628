"""Contamination and sample identity of sorted BAMs from a pileup at known sites, counted on the GPU.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --contamination --contamination_sites V
    python -m hello_amd.contamination --bam B[,P] --ref F --sites V --output_prefix P [--chromosomes a,b] [--q_threshold 10]
                                      [--mapq_threshold 10] [--device N]

Not in the reference; DESIGN.md section 7n defines the rules.  ``read_sites`` reads the sites file; ``observations_of``,
``tables_of``, ``restated``, ``estimate_restated`` and ``identity_restated`` restate the rules in plain Python / NumPy without a GPU;
``Pileup`` binds ``hello_pileup_*`` (hello_amd/csrc/pileup.hip), whose COUNTS equal the restatement integer for integer, and
``estimate_native`` / ``identity_native`` bind the host-only ``hello_contam_*`` (hello_amd/csrc/contam.h).  ``measure`` is the pass
over one BAM: per chromosome one batch of reads per span of at most ``hotspots.MAX_LAUNCH_BASES`` positions -- a read belongs to the
span that holds its start, so no table depends on the spans.  Its result, ``Contamination``, holds the sites and COUNTS per
chromosome and writes the report, the pileup and the ``.npz``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import logging
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, i32, i64, vp
from .bam import Reads
from .gvcf import _bytes_of, counted
from .spans import Handle, measure_spans, save_tables

BINS = ("A", "C", "G", "T", "OTHER", "DEL", "LOWQ")         # the bins of COUNTS [n_sites, 2 strands, 7]
A, C_, G, T, OTHER, DEL, LOWQ = range(7)
SKIP_CAUSES = ("not_snv", "multiallelic", "no_af", "af_out_of_range", "ref_mismatch", "unknown_chromosome", "duplicate_position")
STATUS_NAMES = ("not_counted", "counting", "on_a_site")     # STATUS of the last add, per read
COUNT_NAMES = ("reads_given", "belonging", "counting", "reads_on_a_site", "observations", "n_sites")
STAT_NAMES = COUNT_NAMES + ("sites_ms", "reads_ms")
METRIC_STATS = COUNT_NAMES[1:]                              # what does not depend on the spans
MAX_COUNTING_READS = (1 << 31) - 1
GRID = 501                                                  # alpha_k = k / 1000
DROP = 1.92
MIN_ERROR, MAX_ERROR = 1e-4, 0.1
TWO_PHASE, PLAIN = 0, 1                                     # the forms of the reads kernel (HELLO_PILEUP_FORM)
MAX_SHARE = 1024                                            # the most counting reads of a workgroup (HELLO_PILEUP_SHARE)
PILEUP_HEADER = "#chrom\tpos\tref\talt\taf\tref_fwd\tref_rev\talt_fwd\talt_rev\tother\tdeletions\tlow_quality\n"

_log = logging.getLogger(__name__)
_CODE = np.full(256, 255, np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _CODE[_b | 0x20] = _i


# ------------------------------------------------------------------------------------------------
# the sites file
# ------------------------------------------------------------------------------------------------
class Sites:
    """``per_chromosome[c]``: POS int64 ascending 0-based, REF / ALT uint8 codes 0 - 3, AF float64; ``skipped``: records by cause
    (SKIP_CAUSES); ``records``: the records read."""

    def __init__(self, chromosomes: Sequence[str]):
        self.per_chromosome: Dict[str, Dict[str, np.ndarray]] = {
            c: dict(POS=np.zeros(0, np.int64), REF=np.zeros(0, np.uint8), ALT=np.zeros(0, np.uint8), AF=np.zeros(0, np.float64))
            for c in chromosomes}
        self.skipped: Dict[str, int] = dict.fromkeys(SKIP_CAUSES, 0)
        self.records = 0

    @property
    def n_sites(self) -> int:
        return sum(int(s["POS"].shape[0]) for s in self.per_chromosome.values())


def _af_of(info: str) -> Optional[float]:
    for field in info.split(";"):
        if field.startswith("AF="):
            try:
                return float(field[3:])
            except ValueError:
                return None
    return None


def read_sites(path: str, genome: Dict[str, object], chromosomes: Optional[Sequence[str]] = None) -> Sites:
    """The sites of a VCF, plain or ``.gz``, on the chromosomes of the run (default: every sequence of ``genome``).  A record is a
    site when it has one ALT, REF and ALT are each one of ACGT (case folded), INFO has AF=<float> inside (0, 1) and the reference
    base at POS, folded, is REF; every other record is counted by cause.  Records need not be sorted; of two records at one
    position the first stays."""
    names = list(chromosomes) if chromosomes else list(genome)
    out = Sites(names)
    found: Dict[str, Dict[int, Tuple[int, int, float]]] = {c: {} for c in names}
    refs = {c: _bytes_of(genome[c]) for c in names if c in genome}
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 8:
                raise ValueError(f"{path}: a record of {len(f)} fields, a VCF has 8 at the least")
            out.records += 1
            chromosome, pos, ref, alt, info = f[0], int(f[1]) - 1, f[3], f[4], f[7]
            if chromosome not in refs:
                cause = "unknown_chromosome"
            elif "," in alt:
                cause = "multiallelic"
            elif len(ref) != 1 or len(alt) != 1 or _CODE[ord(ref)] > 3 or _CODE[ord(alt)] > 3:
                cause = "not_snv"
            else:
                af = _af_of(info)
                if af is None:
                    cause = "no_af"
                elif not 0.0 < af < 1.0:
                    cause = "af_out_of_range"
                elif not 0 <= pos < refs[chromosome].shape[0] or int(refs[chromosome][pos]) & 0xDF != ord(ref) & 0xDF:
                    cause = "ref_mismatch"
                elif pos in found[chromosome]:
                    cause = "duplicate_position"
                else:
                    found[chromosome][pos] = (int(_CODE[ord(ref)]), int(_CODE[ord(alt)]), af)
                    continue
            out.skipped[cause] += 1
    for c, sites in found.items():
        at = sorted(sites)
        out.per_chromosome[c] = dict(POS=np.array(at, np.int64), REF=np.array([sites[p][0] for p in at], np.uint8),
                                     ALT=np.array([sites[p][1] for p in at], np.uint8), AF=np.array([sites[p][2] for p in at], np.float64))
    return out


# ------------------------------------------------------------------------------------------------
# the rules, restated: the pileup
# ------------------------------------------------------------------------------------------------
def observations_of(rd: Reads, r: int, is_site: np.ndarray, q_threshold: int = 10) -> List[Tuple[int, int]]:
    """[(site position, bin)] of read ``r`` in reference order.  ``is_site``: bool per position of the chromosome."""
    b0, b1 = int(rd.read_offsets[r]), int(rd.read_offsets[r + 1])
    ops = [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]
    if any(op > 8 for op, _ in ops) or sum(k for op, k in ops if op in (0, 1, 4, 7, 8)) != b1 - b0:
        raise ValueError(f"read {r}: its CIGAR does not consume exactly its {b1 - b0} bases")
    out, pos, i = [], int(rd.ref_starts[r]), b0
    for op, k in ops:
        if op in (0, 7, 8, 2):
            for p in np.flatnonzero(is_site[pos:pos + k]) + pos:
                if op == 2:
                    out.append((int(p), DEL))
                    continue
                base, quality = int(rd.bases[i + p - pos]) & 0xDF, int(rd.quals[i + p - pos])
                out.append((int(p), LOWQ if quality < q_threshold else "ACGT".find(chr(base)) if chr(base) in "ACGT" else OTHER))
            pos += k
            if op != 2:
                i += k
        elif op in (1, 4):
            i += k
        elif op == 3:
            pos += k
    return out


def tables_of(reads: Reads, pos, length: int, lo: int, hi: int, q_threshold: int = 10, mapq_threshold: int = 10) -> Dict[str, object]:
    """One span [lo, hi) of a chromosome of ``length`` bases with the sites ``pos`` and the reads overlapping it -> COUNTS,
    ``counts`` (COUNT_NAMES) and ``status`` (uint8 per read, STATUS_NAMES)."""
    pos = np.asarray(pos, np.int64)
    if not 0 <= lo < hi <= length:
        raise ValueError("a span that leaves the reference")
    is_site = np.zeros(length, bool)
    is_site[pos] = True
    table = np.zeros((pos.shape[0], 2, 7), np.int64)
    status = np.zeros(reads.n_reads, np.uint8)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts.update(reads_given=reads.n_reads, n_sites=int(pos.shape[0]))
    for r in range(reads.n_reads):
        if int(reads.ref_starts[r]) < lo:
            continue
        counts["belonging"] += 1
        if not counted(int(reads.flags[r]), int(reads.mapq[r]), mapq_threshold):
            continue
        counts["counting"] += 1
        seen = observations_of(reads, r, is_site, q_threshold)
        status[r] = 2 if seen else 1
        counts["reads_on_a_site"] += bool(seen)
        counts["observations"] += len(seen)
        strand = int(bool(int(reads.flags[r]) & 0x10))
        for p, which in seen:
            table[int(np.searchsorted(pos, p)), strand, which] += 1
    return dict(COUNTS=table, counts=counts, status=status)


def restated(spans: Sequence[Tuple[Reads, int, int]], pos, length: int, q_threshold: int = 10,
             mapq_threshold: int = 10) -> Tuple[Dict[str, np.ndarray], Dict[str, int]]:
    """({COUNTS}, the counts) of one chromosome given as (reads, lo, hi) span after span, from the restatement."""
    pos = np.asarray(pos, np.int64)
    total = dict(COUNTS=np.zeros((pos.shape[0], 2, 7), np.int64))
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["n_sites"] = int(pos.shape[0])
    for reads, lo, hi in spans:
        part = tables_of(reads, pos, length, lo, hi, q_threshold, mapq_threshold)
        total["COUNTS"] += part["COUNTS"]
        for k, v in part["counts"].items():
            if k != "n_sites":
                counts[k] += v
    return total, counts


def rao_of(counts: np.ndarray, ref: np.ndarray, alt: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per site, over both strands: the count of REF, of ALT and of the two other bases of ACGT (int64 each)."""
    both = np.asarray(counts, np.int64).sum(axis=1)[:, :4]
    at = np.arange(both.shape[0])
    r, a = both[at, np.asarray(ref, np.int64)], both[at, np.asarray(alt, np.int64)]
    return r, a, both.sum(axis=1) - r - a


# ------------------------------------------------------------------------------------------------
# the rules, restated: the estimates
# ------------------------------------------------------------------------------------------------
def error_rate(r, a, o) -> float:
    wrong, total = int(np.sum(o, dtype=np.int64)), int(np.sum(r, dtype=np.int64) + np.sum(a, dtype=np.int64) + np.sum(o, dtype=np.int64))
    if total <= 0:
        return MIN_ERROR
    return min(max(1.5 * float(wrong) / float(total), MIN_ERROR), MAX_ERROR)


def _p_alt(g: int, e):
    return (g / 2) * (1 - e) + (1 - g / 2) * e / 3


def _p_ref(g: int, e):
    return (1 - g / 2) * (1 - e) + (g / 2) * e / 3


def _log_prior(af):
    """[3, n]: Hardy-Weinberg for 0, 1 and 2 ALT copies, log."""
    return np.stack([2 * np.log(1 - af), np.log(af.dtype.type(2)) + np.log(af) + np.log(1 - af), 2 * np.log(af)])


def _lse(parts: List[np.ndarray]) -> np.ndarray:
    m = parts[0]
    for x in parts[1:]:
        m = np.maximum(m, x)
    s = np.zeros_like(m)
    for x in parts:
        s = s + np.exp(x - m)
    return m + np.log(s)


def site_terms(r, a, af, e, dtype=np.float64, k_lo: int = 0, k_hi: int = GRID) -> np.ndarray:
    """[n, k_hi - k_lo]: the per-site term l_i(alpha_k) of every site given (those with r + a > 0 are the ones that count)."""
    t = np.dtype(dtype).type
    r, a, af, e = np.asarray(r).astype(dtype)[:, None], np.asarray(a).astype(dtype)[:, None], np.asarray(af).astype(dtype), t(e)
    alpha = (np.arange(k_lo, k_hi).astype(dtype) / t(1000))[None, :]
    lp = _log_prior(af)
    parts = []
    for g1 in range(3):
        for g2 in range(3):
            lq_ref = np.log((1 - alpha) * _p_ref(g1, e) + alpha * _p_ref(g2, e))
            lq_alt = np.log((1 - alpha) * _p_alt(g1, e) + alpha * _p_alt(g2, e))
            parts.append((lp[g1] + lp[g2])[:, None] + r * lq_ref + a * lq_alt)
    return _lse(parts)


def estimate_restated(r, a, o, af, dtype=np.float64, chunk: int = 64) -> Dict[str, object]:
    """``error_rate``, ``k`` (alpha = k / 1000), ``k_lo``, ``k_hi``, ``LL`` [501] and ``abs_sum`` [501] (the sum of |l_ik| over the
    sites, what a bound on the summation error needs) in ``dtype``; every grid point sums its sites in their order."""
    r, a, o, af = (np.asarray(x) for x in (r, a, o, af))
    e = error_rate(r, a, o)
    used = np.flatnonzero(r + a > 0)
    ll, abs_sum = np.zeros(GRID, dtype), np.zeros(GRID, dtype)
    for k0 in range(0, GRID, chunk):
        terms = site_terms(r[used], a[used], af[used], e, dtype, k0, min(k0 + chunk, GRID))
        if terms.shape[0]:
            ll[k0:k0 + chunk] = np.cumsum(terms, axis=0)[-1]                  # cumsum adds in order; sum would add pairwise
            abs_sum[k0:k0 + chunk] = np.abs(terms).sum(axis=0)
    best = int(np.argmax(ll))
    inside = np.flatnonzero(ll >= ll[best] - np.dtype(dtype).type(DROP))
    return dict(error_rate=e, k=best, k_lo=int(inside[0]), k_hi=int(inside[-1]), LL=ll, abs_sum=abs_sum, n_used=int(used.shape[0]))


def identity_restated(r1, a1, o1, r2, a2, o2, af, dtype=np.float64) -> Tuple[object, int]:
    """(LOD, sites used): the log odds of one person against two unrelated people over the sites with r + a > 0 in both."""
    t = np.dtype(dtype).type
    r1, a1, o1, r2, a2, o2, af = (np.asarray(x) for x in (r1, a1, o1, r2, a2, o2, af))
    e1, e2 = t(error_rate(r1, a1, o1)), t(error_rate(r2, a2, o2))
    used = np.flatnonzero((r1 + a1 > 0) & (r2 + a2 > 0))
    if used.shape[0] == 0:
        return t(0), 0
    lp = _log_prior(af[used].astype(dtype))
    like = lambda r, a, e: [r[used].astype(dtype) * np.log(_p_ref(g, e)) + a[used].astype(dtype) * np.log(_p_alt(g, e)) for g in range(3)]  # noqa: E731
    l1, l2 = like(r1, a1, e1), like(r2, a2, e2)
    terms = (_lse([lp[g] + l1[g] + l2[g] for g in range(3)]) - _lse([lp[g] + l1[g] for g in range(3)])
             - _lse([lp[g] + l2[g] for g in range(3)]))
    return np.cumsum(terms)[-1], int(used.shape[0])


def verdict(lod: float, used: int) -> str:
    return "undetermined" if used == 0 or lod == 0 else "same_sample" if lod > 0 else "different_sample"


# ------------------------------------------------------------------------------------------------
# the library
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_pileup_create", [vp, i64, i64, i32, i32, i32, C.POINTER(vp)]),
    ("hello_pileup_option", [vp, i32, i32]),
    ("hello_pileup_add", [vp] + READS + [i64, i64, i64]),
    ("hello_pileup_array", ARRAY_GETTER),
    ("hello_pileup_stats", STATS_GETTER),
    ("hello_pileup_free", [vp], None),
    ("hello_contam_estimate", [vp, vp, vp, vp, i64, vp]),
    ("hello_contam_identity", [vp, vp, vp, vp, vp, vp, vp, i64, vp]),
)


def _lib():
    return bind(_PROTOTYPES)


def _i64(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.int64)


def estimate_native(r, a, o, af) -> Dict[str, object]:
    """``estimate_restated`` from ``hello_contam_estimate`` (host only: no device is opened)."""
    r, a, o, af = _i64(r), _i64(a), _i64(o), np.ascontiguousarray(af, np.float64)
    out = np.zeros(4 + GRID, np.float64)
    check(_lib().hello_contam_estimate(r.ctypes.data, a.ctypes.data, o.ctypes.data, af.ctypes.data, int(r.shape[0]), out.ctypes.data))
    return dict(error_rate=float(out[0]), k=int(out[1]), k_lo=int(out[2]), k_hi=int(out[3]), LL=out[4:].copy(),
                n_used=int(np.count_nonzero(r + a > 0)))


def identity_native(r1, a1, o1, r2, a2, o2, af) -> Tuple[float, int]:
    arrays = [_i64(x) for x in (r1, a1, o1, r2, a2, o2)] + [np.ascontiguousarray(af, np.float64)]
    out = np.zeros(2, np.float64)
    check(_lib().hello_contam_identity(*[x.ctypes.data for x in arrays], int(arrays[0].shape[0]), out.ctypes.data))
    return float(out[0]), int(out[1])


class Pileup(Handle):
    """One (BAM, chromosome)'s ``hello_pileup`` handle: ``add`` takes the reads overlapping a span, ``arrays`` gives COUNTS and the
    STATUS of the last ``add``.  ``form``: TWO_PHASE (the default) or PLAIN; ``share``: the counting reads of a workgroup of the
    reads kernel, 1 to MAX_SHARE, or 0 (the default: every ``add`` sizes it) -- the same bytes whatever they are."""
    NAME, STAT_NAMES, TIMES = "pileup", STAT_NAMES, STAT_NAMES[len(COUNT_NAMES):]
    ARRAYS = (("COUNTS", 0, np.int64, (-1, 2, 7)), ("STATUS", 1, np.uint8, None))

    def __init__(self, pos, length: int, q_threshold: int = 10, mapq_threshold: int = 10, device: int = 0, form: int = TWO_PHASE,
                 share: int = 0):
        pos = _i64(pos)
        super().__init__(_lib())
        check(self._lib.hello_pileup_create(pos.ctypes.data, int(pos.shape[0]), int(length), int(q_threshold), int(mapq_threshold),
                                            int(device), C.byref(self._h)))
        try:
            if form != TWO_PHASE:
                check(self._lib.hello_pileup_option(self._h, 0, int(form)))
            if share:
                check(self._lib.hello_pileup_option(self._h, 1, int(share)))
        except Exception:
            self.close()
            raise

    def add(self, reads: Reads, lo: int, hi: int) -> None:
        check(self._lib.hello_pileup_add(self._h, *reads.pointers(reads.hp), int(reads.n_reads), int(lo), int(hi)))


def counted_on_gpu(spans: Sequence[Tuple[Reads, int, int]], pos, length: int, q_threshold: int = 10, mapq_threshold: int = 10,
                   device: int = 0, form: int = TWO_PHASE, share: int = 0) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
    """``restated`` on the GPU: ({COUNTS, STATUS of the last span}, the statistics of ``hello_pileup_stats``)."""
    with Pileup(pos, length, q_threshold, mapq_threshold, device, form, share) as pileup:
        for reads, lo, hi in spans:
            pileup.add(reads, lo, hi)
        return pileup.arrays(), pileup.stats()


# ------------------------------------------------------------------------------------------------
# the contamination of one BAM
# ------------------------------------------------------------------------------------------------
class Contamination:
    """``tables[chromosome]``: POS, REF, ALT, AF of its sites, COUNTS int64 [n, 2, 7] and STATS (int64, METRIC_STATS); ``skipped``
    and ``records`` of the sites file.  ``native``: the estimates come from the library (else from the NumPy restatement)."""

    def __init__(self, sites: Optional[Sites] = None, native: bool = True):
        self.tables: Dict[str, Dict[str, np.ndarray]] = {}
        self.skipped: Dict[str, int] = dict(sites.skipped) if sites else dict.fromkeys(SKIP_CAUSES, 0)
        self.records = sites.records if sites else 0
        self.native = native

    def set(self, chromosome: str, site: Dict[str, np.ndarray], counts_table, counts: Dict[str, float]) -> None:
        self.tables[chromosome] = dict(POS=np.asarray(site["POS"], np.int64), REF=np.asarray(site["REF"], np.uint8),
                                       ALT=np.asarray(site["ALT"], np.uint8), AF=np.asarray(site["AF"], np.float64),
                                       COUNTS=np.asarray(counts_table, np.int64).reshape(-1, 2, 7),
                                       STATS=np.array([int(counts[k]) for k in METRIC_STATS], np.int64))

    def total(self) -> Dict[str, int]:
        return {k: sum(int(t["STATS"][i]) for t in self.tables.values()) for i, k in enumerate(METRIC_STATS)}

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(r, a, o, af) of every site, the chromosomes one behind the other."""
        parts = [rao_of(t["COUNTS"], t["REF"], t["ALT"]) + (t["AF"],) for t in self.tables.values()]
        cat = lambda k, dtype: np.concatenate([p[k] for p in parts] + [np.zeros(0, dtype)]).astype(dtype)      # noqa: E731
        return cat(0, np.int64), cat(1, np.int64), cat(2, np.int64), cat(3, np.float64)

    def estimate(self) -> Dict[str, object]:
        return (estimate_native if self.native else estimate_restated)(*self.arrays())

    def report(self) -> str:
        """The text of ``<prefix>.txt``."""
        total, est = self.total(), self.estimate()
        lines = ["sites_read\t%d" % self.records] + ["sites_skipped_%s\t%d" % (k, self.skipped[k]) for k in SKIP_CAUSES]
        lines += ["sites\t%d" % total["n_sites"], "sites_with_coverage\t%d" % est["n_used"],
                  "reads_not_counted\t%d" % (total["belonging"] - total["counting"]), "reads_counting\t%d" % total["counting"],
                  "reads_on_a_site\t%d" % total["reads_on_a_site"], "observations\t%d" % total["observations"],
                  "error_rate\t%.6f" % est["error_rate"], "contamination\t%.3f" % (est["k"] / 1000),
                  "contamination_lo\t%.3f" % (est["k_lo"] / 1000), "contamination_hi\t%.3f" % (est["k_hi"] / 1000),
                  "mean_depth_at_sites\t%.3f" % (total["observations"] / total["n_sites"] if total["n_sites"] else 0.0)]
        return "\n".join(lines) + "\n"

    def pileup_text(self) -> str:
        """The text of ``<prefix>.pileup.tsv``: a header, then a line per site with coverage."""
        out = [PILEUP_HEADER]
        for c, t in self.tables.items():
            n = t["COUNTS"]
            for s in np.flatnonzero(n.sum(axis=(1, 2))):
                ref, alt = int(t["REF"][s]), int(t["ALT"][s])
                other = int(n[s, :, :5].sum() - n[s, :, ref].sum() - n[s, :, alt].sum())
                out.append("%s\t%d\t%s\t%s\t%.6g\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
                    c, int(t["POS"][s]) + 1, "ACGT"[ref], "ACGT"[alt], float(t["AF"][s]), n[s, 0, ref], n[s, 1, ref], n[s, 0, alt],
                    n[s, 1, alt], other, int(n[s, :, DEL].sum()), int(n[s, :, LOWQ].sum())))
        return "".join(out)

    def save(self, path: str) -> str:
        names = list(self.tables)
        out = dict(chromosomes=np.array(names, dtype=np.str_), SKIPPED=np.array([self.skipped[k] for k in SKIP_CAUSES], np.int64),
                   RECORDS=np.array([self.records], np.int64))
        for i, c in enumerate(names):
            for name, a in self.tables[c].items():
                out["%s_%d" % (name, i)] = a
        return save_tables(path, out)

    @classmethod
    def load(cls, path: str, native: bool = True) -> "Contamination":
        with np.load(path, allow_pickle=False) as z:
            out = cls(native=native)
            out.skipped = dict(zip(SKIP_CAUSES, (int(v) for v in z["SKIPPED"])))
            out.records = int(z["RECORDS"][0])
            for i, c in enumerate(str(c) for c in z["chromosomes"]):
                out.tables[c] = {name: z["%s_%d" % (name, i)] for name in ("POS", "REF", "ALT", "AF", "COUNTS", "STATS")}
        return out

    def write_all(self, prefix: str) -> List[str]:
        """``<prefix>.txt``, ``<prefix>.pileup.tsv`` and ``<prefix>.npz``."""
        for suffix, text in ((".txt", self.report()), (".pileup.tsv", self.pileup_text())):
            with open(prefix + suffix, "w") as fh:
                fh.write(text)
        return [prefix + ".txt", prefix + ".pileup.tsv", self.save(prefix + ".npz")]


def identity_of(first: Contamination, second: Contamination) -> Tuple[float, int, str]:
    """(LOD, sites used, verdict) of two BAMs measured at the same sites."""
    (r1, a1, o1, af), (r2, a2, o2, af2) = first.arrays(), second.arrays()
    if af.shape != af2.shape or not np.array_equal(af, af2):
        raise ValueError("the two BAMs were not measured at the same sites")
    lod, used = (identity_native if first.native else identity_restated)(r1, a1, o1, r2, a2, o2, af)
    return float(lod), used, verdict(float(lod), used)


def identity_text(lod: float, used: int, said: str) -> str:
    return "sites_used\t%d\nlod\t%.3f\nverdict\t%s\n" % (used, lod, said)


def write_identity(path: str, first: Contamination, second: Contamination) -> str:
    with open(path, "w") as fh:
        fh.write(identity_text(*identity_of(first, second)))
    return path


def measure(bam: str, fasta, chromosomes: Optional[Sequence[str]], sites: Sites, q_threshold: int = 10, mapq_threshold: int = 10,
            device: int = 0, stats: Optional[dict] = None, max_span: Optional[int] = None, restatement: bool = False,
            form: int = TWO_PHASE, share: int = 0) -> Contamination:
    """The pileup of one BAM at ``sites``, chromosome after chromosome (default: every sequence of the FASTA).  ``fasta``: a path, or
    {chromosome: sequence}; ``restatement``: from the plain-Python rules instead of the GPU and the library.  ``stats``: the library's
    kernel times and the seconds of decoding (``decode_s``), of the library's calls (``device_s``) and of the whole pass
    (``total_s``) are added."""
    out = Contamination(sites, native=not restatement)
    at = sites.per_chromosome
    measure_spans(bam, fasta, chromosomes, max_span, stats, restatement,
                  open_handle=lambda c, ref: Pileup(at[c]["POS"], ref.shape[0], q_threshold, mapq_threshold, device, form, share),
                  restated=lambda c, ref, spans: restated(spans, at[c]["POS"], ref.shape[0], q_threshold, mapq_threshold),
                  done=lambda c, ref, tables, counts: out.set(c, at[c], tables["COUNTS"], counts))
    return out


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Contamination and sample identity of coordinate-sorted BAMs from a pileup at known sites, counted on the GPU")
    p.add_argument("--bam", required=True, help="The BAM (with its .bai, or scanned); B,P: two BAMs, whose identity is also reported")
    p.add_argument("--ref", required=True, help="Reference FASTA")
    p.add_argument("--sites", required=True, help="A VCF (plain or .gz) of biallelic SNVs with INFO AF")
    p.add_argument("--output_prefix", required=True,
                   help="Writes <prefix>.txt, .pileup.tsv and .npz; with two BAMs <prefix>.1.* and <prefix>.2.* and <prefix>.identity.txt")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes (default: every sequence of the FASTA)")
    p.add_argument("--q_threshold", type=int, default=10, help="A base below it goes to the low-quality bin")
    p.add_argument("--mapq_threshold", type=int, default=10, help="A read below it does not count")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> List[str]:
    from .call import read_fasta
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    chromosomes = args.chromosomes.split(",") if args.chromosomes else None
    genome = read_fasta(args.ref, chromosomes)
    sites = read_sites(args.sites, genome, chromosomes)
    bams = args.bam.split(",")
    if not 1 <= len(bams) <= 2:
        raise SystemExit("--bam takes one BAM, or two separated by a comma")
    written, found = [], []
    for n, bam in enumerate(bams):
        stats: dict = {}
        got = measure(bam, genome, chromosomes, sites, args.q_threshold, args.mapq_threshold, args.device, stats)
        found.append(got)
        written += got.write_all(args.output_prefix + (".%d" % (n + 1) if len(bams) > 1 else ""))
        total, est = got.total(), got.estimate()
        _log.info("%s: %d sites, %d reads counting, %d observations, contamination %.3f [%.3f, %.3f] (kernels %.1f ms)", os.path.basename(bam),
                  total["n_sites"], total["counting"], total["observations"], est["k"] / 1000, est["k_lo"] / 1000, est["k_hi"] / 1000,
                  stats.get("sites_ms", 0.0) + stats.get("reads_ms", 0.0))
    if len(found) == 2:
        written.append(write_identity(args.output_prefix + ".identity.txt", *found))
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
