"""Haplotags from a phased VCF: ``hp`` (1, 2 or 0) and ``ps`` for every read of any read set, on the GPU.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --include_hp --haplotag_vcf phased.vcf
    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --include_hp --haplotag

Not in the reference; DESIGN.md section 7h defines the rule.  ``phased``, ``phased_records`` and ``haplotags_restated`` restate it
in plain Python without a GPU -- the counted reads, the candidate records and the observation at a record are those of section 7g
and come from ``hello_amd.phase`` (``observe``, ``reference_end``), not from a second copy; ``Haplotagger`` binds
``hello_haplotag_*`` (hello_amd/csrc/haplotag.hip), which equals the restatement integer for integer: one device-resident record
table per chromosome, one fused launch per read set.  The candidate stages take a ``Haplotagger`` as ``tagger=`` and pass the
reads they fetch through ``retag`` before they look for sites.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import logging
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import phase
from ._abi import READS, STATS_GETTER, bind, check, handle_stats, i32, i64, vp
from .bam import Reads
from .gvcf import counted

STAT_NAMES = ("records", "calls", "reads", "reads_counted", "reads_hp1", "reads_hp2", "kernel_ms", "plan_ms", "total_ms")

_log = logging.getLogger(__name__)


class PhasedRecord(NamedTuple):
    """A phased record: its span [start, end) = [POS - 1, POS - 1 + len(REF)), the genotype a|b, the allele of haplotype 1
    (``allele_a``, allele a of the line) and of haplotype 2 (``allele_b``), and its phase set.  The first six fields are those of
    ``phase.Record``, so ``phase.observe`` reads it as one: observation 0 is haplotype 1, observation 1 is haplotype 2."""
    start: int
    end: int
    a: int
    b: int
    allele_a: bytes
    allele_b: bytes
    ps: int

    @property
    def pos(self) -> int:
        return self.start + 1


# ------------------------------------------------------------------------------------------------
# the rule, restated
# ------------------------------------------------------------------------------------------------
def _parse(line: bytes) -> Tuple[Optional[PhasedRecord], bool]:
    """(the phased record of one VCF data line or None, whether the line is ``a|b`` over ACGT alleles but has no positive PS)."""
    f = line.rstrip(b"\r\n").split(b"\t")
    if len(f) < 10:
        return None, False
    sample = f[9].split(b":")
    if sample[0].count(b"|") != 1:
        return None, False
    rec = phase.phasable(b"\t".join(f[:9] + [sample[0].replace(b"|", b"/")]))      # the allele test of section 7g, on a/b
    if rec is None:
        return None, False
    keys = f[8].split(b":")
    at = keys.index(b"PS") if b"PS" in keys else -1
    value = sample[at] if 0 <= at < len(sample) else b""
    if not value.isdigit() or int(value) <= 0:
        return None, True
    return PhasedRecord(*rec, int(value)), False


def phased(line: bytes) -> Optional[PhasedRecord]:
    """The phased record of one VCF data line, or None when the line is ignored: the first field of its sample column is ``a|b``
    with integers a != b that name alleles of the line, both allele strings are ACGT only after upper-casing, and its FORMAT has
    a ``PS`` key whose sample value is a positive integer."""
    return _parse(line)[0]


def phased_records(vcf_path: str, chromosomes: Optional[Sequence[str]] = None, stats: Optional[dict] = None) -> Dict[str, List[PhasedRecord]]:
    """{chromosome: its phased records in file order} of ``chromosomes`` (default: every chromosome of the file).  Records that
    are not sorted by start within a chromosome are refused.  Lines with ``a|b`` but no positive PS are ignored, counted into
    ``stats["lines_without_ps"]`` and logged once."""
    out: Dict[str, List[PhasedRecord]] = {}
    without = 0
    with open(vcf_path, "rb") as fh:
        for line in fh:
            if line.startswith(b"#"):
                continue
            c = line.split(b"\t", 1)[0].decode()
            if chromosomes and c not in chromosomes:
                continue
            rec, no_ps = _parse(line)
            without += no_ps
            if rec is None:
                continue
            mine = out.setdefault(c, [])
            if mine and rec.start < mine[-1].start:
                raise ValueError(f"{vcf_path}: the records of {c} are not sorted by position (POS {rec.pos} after {mine[-1].pos})")
            mine.append(rec)
    if without:
        _log.warning("%s: %d lines are phased (a|b) without a positive PS and were ignored", vcf_path, without)
    if stats is not None:
        stats["lines_without_ps"] = stats.get("lines_without_ps", 0) + without
        stats["phased_records"] = stats.get("phased_records", 0) + sum(len(v) for v in out.values())
    return out


def _single(reads: Union[Reads, Sequence[Reads]]) -> Reads:
    return reads if isinstance(reads, Reads) else phase._one(reads)


def haplotags_restated(reads: Union[Reads, Sequence[Reads]], records: Sequence[PhasedRecord], q_threshold: int = 10,
                       mapq_threshold: int = 10) -> Tuple[np.ndarray, np.ndarray]:
    """(hp uint8 [reads], ps int64 [reads]) of one read set, or of one or two one after the other.  A counted read's candidates
    are the records with ref_start <= start < ref_end; its set is the PS of its first observation among them, in record order;
    over its observations at records of that set, n1 counts observation 0 and n2 observation 1; hp is 1, 2 or 0 for n1 > n2,
    n2 > n1, or a tie or no observation; ps is that set, also at a tie, and 0 without an observation."""
    rd = _single(reads)
    starts = phase._check_sorted(records)
    hp, ps = np.zeros(rd.n_reads, np.uint8), np.zeros(rd.n_reads, np.int64)
    for r in range(rd.n_reads):
        if not counted(int(rd.flags[r]), int(rd.mapq[r]), mapq_threshold):
            continue
        if sum(k for op, k in phase._ops(rd, r) if op in (0, 1, 4, 7, 8)) > int(rd.read_offsets[r + 1] - rd.read_offsets[r]):
            raise ValueError(f"read {r}: its CIGAR consumes more bases than it has")
        first = int(np.searchsorted(starts, int(rd.ref_starts[r]), "left"))
        last = int(np.searchsorted(starts, phase.reference_end(rd, r), "left"))
        mine, count = 0, [0, 0]
        for t in range(first, last):
            o = phase.observe(rd, r, records[t], q_threshold)
            if o < 0:
                continue
            if not mine:
                mine = records[t].ps
            if records[t].ps == mine:
                count[o] += 1
        hp[r] = 1 if count[0] > count[1] else 2 if count[1] > count[0] else 0
        ps[r] = mine
    return hp, ps


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_haplotag_create", [vp, vp, vp, vp, vp, i64, i32, C.POINTER(vp)]),
    ("hello_haplotag_reads", [vp] + READS + [i64, i32, i32, vp, vp]),
    ("hello_haplotag_stats", STATS_GETTER),
    ("hello_haplotag_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


def record_table(records: Sequence[PhasedRecord]):
    """The arrays ``hello_haplotag_create`` takes: (starts, ends, alleles, allele offsets [2 n + 1], ps)."""
    text = [x for rec in records for x in (rec.allele_a, rec.allele_b)]
    return (np.array([rec.start for rec in records], np.int64), np.array([rec.end for rec in records], np.int64),
            np.frombuffer(b"".join(text), np.uint8), np.concatenate([[0], np.cumsum([len(x) for x in text])]).astype(np.int64),
            np.array([rec.ps for rec in records], np.int64))


class Haplotagger:
    """The phased records of a VCF, and per chromosome one ``hello_haplotag`` handle (its table on the device), created when the
    chromosome's first reads arrive.  ``tag`` -> (hp, ps) of a read set; ``retag`` -> the read set with ``hp`` replaced;
    ``stats``: the handles' statistics summed; ``close`` frees the handles.  ``records``: {chromosome: [PhasedRecord]} instead of
    a file."""

    def __init__(self, vcf_path: Optional[str], chromosomes: Optional[Sequence[str]] = None, q_threshold: int = 10,
                 mapq_threshold: int = 10, device: int = 0, records: Optional[Dict[str, Sequence[PhasedRecord]]] = None):
        self._extra: Dict[str, float] = {}
        self.records = phased_records(vcf_path, chromosomes, self._extra) if records is None else {c: list(v) for c, v in records.items()}
        for recs in self.records.values():
            phase._check_sorted(recs)
        self.q_threshold, self.mapq_threshold, self.device = int(q_threshold), int(mapq_threshold), int(device)
        self._lib = _lib()
        self._handles: Dict[str, C.c_void_p] = {}
        self._done = {name: 0.0 for name in STAT_NAMES}             # of the handles already freed, and of reads never launched

    def _handle(self, chromosome: str) -> C.c_void_p:
        h = self._handles.get(chromosome)
        if h is None:
            table = record_table(self.records[chromosome])
            h = C.c_void_p()
            check(self._lib.hello_haplotag_create(*(a.ctypes.data for a in table), len(self.records[chromosome]), self.device,
                                                  C.byref(h)))
            self._handles[chromosome] = h
        return h

    def tag(self, chromosome: str, reads: Union[Reads, Sequence[Reads]]) -> Tuple[np.ndarray, np.ndarray]:
        """(hp uint8, ps int64) of every read of ``reads`` (one read set, or one or two one after the other) on ``chromosome``.  A
        chromosome without phased records gives zeros without a launch."""
        rd = _single(reads)
        hp, ps = np.zeros(rd.n_reads, np.uint8), np.zeros(rd.n_reads, np.int64)
        if not self.records.get(chromosome):
            self._done["calls"] += 1
            self._done["reads"] += rd.n_reads
            return hp, ps
        check(self._lib.hello_haplotag_reads(self._handle(chromosome), *rd.pointers(rd.hp), int(rd.n_reads), self.q_threshold,
                                             self.mapq_threshold, hp.ctypes.data, ps.ctypes.data))
        return hp, ps

    def retag(self, chromosome: str, reads: Reads) -> Reads:
        """``reads`` with ``hp`` replaced by the haplotags (the tags the BAM carried are dropped)."""
        return dataclasses.replace(reads, hp=self.tag(chromosome, reads)[0])

    @property
    def stats(self) -> Dict[str, float]:
        total = dict(self._done, **self._extra)
        for h in self._handles.values():
            for k, v in handle_stats(self._lib.hello_haplotag_stats, h, STAT_NAMES).items():
                total[k] += v
        total["records"] = float(sum(len(v) for v in self.records.values()))
        return total

    def close(self) -> None:
        self._done = {k: v for k, v in self.stats.items() if k in STAT_NAMES}
        for h in self._handles.values():
            self._lib.hello_haplotag_free(h)
        self._handles = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
