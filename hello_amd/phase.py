"""Read-backed phasing: a phased VCF beside the final VCF, and a haplotype for every read.

    python -m hello_amd.call --from_bam | --from_bams [--resident] ... --phase [--phase_window 8] [--phase_min_margin 2]
    python -m hello_amd.phase --vcf results.output.vcf --bam illumina.bam[,pacbio.bam] --output out.phased.vcf

Not in the reference; DESIGN.md section 7g defines the rules.  ``phasable``, ``observe``, ``slots_of``, ``links_of``, ``chain``,
``haplotags_of``, ``phased_line`` and ``phased_header`` restate them in plain Python / NumPy without a GPU; ``find_observations``,
``chain_native`` and ``find_haplotags`` bind ``hello_phase_*`` (hello_amd/csrc/phase.hip), which equal the restatement integer for
integer; ``write_phased_vcf`` is the driver pass: its own walk over the BAM(s) after scoring, one batch of reads per span of at
most ``hotspots.MAX_LAUNCH_BASES`` positions (a read belongs to the span that holds its start), the spans' links added on the
host, one chain per chromosome.

``--phase_fragments`` (off by default) makes the two mates of a read pair one fragment: ``join_mates`` /
``mates_of``, ``fragment_observations`` and the ``mate`` argument of ``links_of`` and ``haplotags_of`` restate the rules;
``Phaser.fragments`` binds ``hello_phase_fragments`` (the pair and fragment-link kernels), ``Phaser.tag(..., fragments=True)``
``hello_phase_tag_fragments``.  The driver collects name_hash, flags and source span after span and joins once per chromosome, so
mates in different spans are joined too.
"""
from __future__ import annotations

import argparse
import ctypes as C
import logging
import sys
import time
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, READS, STATS_GETTER, bind, check, handle_stats, i32, i64, vp
from .bam import BamFile, Reads
from .gvcf import counted
from .spans import Handle, adder, span_step

NONE = -1
MAX_WINDOW = 32                             # HELLO_PHASE_MAX_WINDOW
DEFAULT_WINDOW = 8
DEFAULT_MIN_MARGIN = 2
PS_HEADER = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set: POS of its first record">\n'
SLOTS, SLOT_OFFSETS, FIRST, LINKS, HP, PS = range(6)
MATE, FRAGMENT_LINKS = 6, 7
STAT_NAMES = ("records", "reads", "reads_counted", "slots", "observe_ms", "link_ms", "tag_ms", "plan_ms", "total_ms")
FRAGMENT_STAT_NAMES = ("pairs", "groups_refused", "pair_ms", "fragment_link_ms", "fragment_tag_ms")

_log = logging.getLogger(__name__)
_ACGT = frozenset(b"ACGT")


class Record(NamedTuple):
    """A phasable record: its span [start, end) = [POS - 1, POS - 1 + len(REF)), the genotype a/b and the two allele strings."""
    start: int
    end: int
    a: int
    b: int
    allele_a: bytes
    allele_b: bytes

    @property
    def pos(self) -> int:
        return self.start + 1


# ------------------------------------------------------------------------------------------------
# the rules, restated
# ------------------------------------------------------------------------------------------------
def phasable(line: bytes) -> Optional[Record]:
    """The record of one VCF data line, or None when it passes through: the first field of its sample column is ``a/b`` with
    integers a != b that name alleles of the line, and both allele strings are ACGT only after upper-casing."""
    f = line.rstrip(b"\r\n").split(b"\t")
    if len(f) < 10:
        return None
    gt = f[9].split(b":", 1)[0].split(b"/")
    if len(gt) != 2 or not all(g.isdigit() for g in gt):
        return None
    a, b = int(gt[0]), int(gt[1])
    alleles = [f[3].upper()] + [x.upper() for x in f[4].split(b",")]
    if a == b or max(a, b) >= len(alleles):
        return None
    if not all(alleles[k] and set(alleles[k]) <= _ACGT for k in (a, b)):
        return None
    start = int(f[1]) - 1
    return Record(start, start + len(f[3]), a, b, alleles[a], alleles[b])


def _ops(rd: Reads, r: int) -> List[Tuple[int, int]]:
    return [(int(c) & 15, int(c) >> 4) for c in rd.cigars[int(rd.cigar_offsets[r]):int(rd.cigar_offsets[r + 1])]]


def reference_end(rd: Reads, r: int) -> int:
    """``ref_start`` plus the reference bases the CIGAR consumes (M, D, N, =, X)."""
    return int(rd.ref_starts[r]) + sum(n for op, n in _ops(rd, r) if op in (0, 2, 3, 7, 8))


def observe_why(rd: Reads, r: int, rec: Record, q_threshold: int = 10) -> Tuple[int, str]:
    """What read ``r`` shows at ``rec`` -- 0 (allele a), 1 (allele b) or NONE -- and the cause of a NONE: ``"end"`` (no aligned base
    behind the span), ``"N"``, ``"neither"`` or ``"quality"``.  The read is taken as counted and the record as a candidate."""
    ops = _ops(rd, r)
    b0 = int(rd.read_offsets[r])
    p, i = int(rd.ref_starts[r]), 0
    if not (p <= rec.start and rec.end < reference_end(rd, r)):
        return NONE, "end"
    text, quals = bytearray(), []

    def append(j0, j1):
        text.extend(bytes(rd.bases[b0 + j0:b0 + j1] & 0xDF))
        quals.extend(int(q) for q in rd.quals[b0 + j0:b0 + j1])
    for op, n in ops:
        if op in (0, 7, 8):
            j0, j1 = max(rec.start - p, 0), min(rec.end - p, n)
            if j1 > j0:
                append(i + j0, i + j1)
            p += n
            i += n
        elif op == 1:
            if rec.start <= p - 1 < rec.end:          # joined to the base on its left, whatever operation put the cursor there
                append(i, i + n)
            i += n
        elif op == 2:
            p += n
        elif op == 3:
            if p < rec.end and p + n > rec.start:
                return NONE, "N"
            p += n
        elif op == 4:
            i += n
    o = 0 if bytes(text) == rec.allele_a else 1 if bytes(text) == rec.allele_b else NONE
    if o == NONE:
        return NONE, "neither"
    if min(quals) < q_threshold:
        return NONE, "quality"
    return o, ""


def observe(rd: Reads, r: int, rec: Record, q_threshold: int = 10) -> int:
    return observe_why(rd, r, rec, q_threshold)[0]


def _one(reads: Sequence[Reads]) -> Reads:
    if not 1 <= len(reads) <= 2:
        raise ValueError("one or two read sets (BAM files)")
    return reads[0] if len(reads) == 1 else Reads.concat(list(reads))[0]


def _check_sorted(records: Sequence[Record]) -> np.ndarray:
    starts = np.array([rec.start for rec in records], np.int64)
    if (np.diff(starts) < 0).any():
        raise ValueError("records are not sorted by position")
    return starts


def counted_mask(rd: Reads, mapq_threshold: int = 10) -> np.ndarray:
    """bool [reads]: ``gvcf.counted`` of every read."""
    return np.array([counted(int(f), int(m), mapq_threshold) for f, m in zip(rd.flags, rd.mapq)], bool)


def slots_of(reads: Sequence[Reads], records: Sequence[Record], q_threshold: int = 10, mapq_threshold: int = 10):
    """(slots int8, slot_offsets int64 [reads + 1], first int64 [reads]) over the read sets one after the other: per counted read one
    slot per record with ref_start <= A < ref_end, in record order; an uncounted read has none."""
    rd = _one(reads)
    starts = _check_sorted(records)
    slots: List[int] = []
    offsets, first = [0], []
    for r in range(rd.n_reads):
        f = n = 0
        if counted(int(rd.flags[r]), int(rd.mapq[r]), mapq_threshold):
            if sum(k for op, k in _ops(rd, r) if op in (0, 1, 4, 7, 8)) > int(rd.read_offsets[r + 1] - rd.read_offsets[r]):
                raise ValueError(f"read {r}: its CIGAR consumes more bases than it has")
            f = int(np.searchsorted(starts, int(rd.ref_starts[r]), "left"))
            n = max(int(np.searchsorted(starts, reference_end(rd, r), "left")) - f, 0)
            slots += [observe(rd, r, records[t], q_threshold) for t in range(f, f + n)]
        first.append(f)
        offsets.append(offsets[-1] + n)
    return np.array(slots, np.int8), np.array(offsets, np.int64), np.array(first, np.int64)


def join_mates(name_hash, flags, source, is_counted):
    """(mate int64 [reads], {pairs, groups_refused}) -- section 7i: the counted reads grouped by (source, name_hash); a group of
    exactly two reads that both have flag 0x1, one with ``flag & 0xC0 == 0x40`` and one with ``== 0x80``, is a pair and each
    read's mate is the other's index; every other read has -1.  ``groups_refused``: the groups of two or more left apart."""
    groups: Dict[Tuple[int, int], List[int]] = {}
    for r in range(len(flags)):
        if is_counted[r]:
            groups.setdefault((int(source[r]), int(name_hash[r])), []).append(r)
    mate = np.full(len(flags), -1, np.int64)
    pairs = refused = 0
    for members in groups.values():
        kinds = sorted(int(flags[r]) & 0xC0 if int(flags[r]) & 0x1 else 0 for r in members)
        if kinds == [0x40, 0x80]:
            mate[members[0]], mate[members[1]] = members[1], members[0]
            pairs += 1
        elif len(members) >= 2:
            refused += 1
    return mate, dict(pairs=pairs, groups_refused=refused)


def mates_of(reads: Sequence[Reads], mapq_threshold: int = 10, details: Optional[dict] = None) -> np.ndarray:
    """int64 [reads]: ``join_mates`` over the read sets one after the other, a read's source being its set.  ``details``: filled
    with pairs and groups_refused."""
    if not 1 <= len(reads) <= 2:
        raise ValueError("one or two read sets (BAM files)")
    rd, source = Reads.concat(list(reads))
    mate, counts = join_mates(rd.name_hash, rd.flags, source, counted_mask(rd, mapq_threshold))
    if details is not None:
        details.update(counts)
    return mate


def fragment_observations(slots, slot_offsets, first, mate):
    """(slots int8, slot_offsets int64 [reads + 1], first int64 [reads]) of every read's FRAGMENT -- itself, or itself and its
    mate: one value F(t) per record from the first to the last candidate record of either read.  F(t) is none where no slot
    covers t (the gap between the mates), the slot's value where one read covers t, and with two the common value, the observed
    one where only one observed, none where they disagree.  Both mates of a pair get the same arrays."""
    out: List[int] = []
    offsets, lows = [0], []
    for r in range(len(first)):
        ranges = [(int(first[x]), int(slot_offsets[x]), int(slot_offsets[x + 1] - slot_offsets[x]))
                  for x in ((r,) if mate[r] < 0 else (r, int(mate[r])))]
        ranges = [x for x in ranges if x[2] > 0]
        lo = min((f for f, _, _ in ranges), default=int(first[r]))
        hi = max((f + k for f, _, k in ranges), default=lo)
        for t in range(lo, hi):
            seen = {int(slots[s + t - f]) for f, s, k in ranges if f <= t < f + k} - {NONE}
            out.append(seen.pop() if len(seen) == 1 else NONE)
        lows.append(lo)
        offsets.append(offsets[-1] + hi - lo)
    return np.array(out, np.int8), np.array(offsets, np.int64), np.array(lows, np.int64)


def pair_table_size(n_counted: int) -> int:
    """Slots of the pair kernels' open-addressing table: the power of two that is at least twice the counted reads (and 2)."""
    size = 2
    while size < 2 * n_counted:
        size <<= 1
    return size


def pair_table_slot(name_hash, source, size: int) -> np.ndarray:
    """uint32: the first slot the pair kernels probe for (name_hash, source) in a table of ``size`` slots (phase_pair.h: pair_slot)."""
    x = np.asarray(name_hash, np.uint64)
    x = x ^ (x >> np.uint64(29))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(32))
    return (((x & np.uint64(0xFFFFFFFF)) + np.asarray(source, np.uint64)) & np.uint64(size - 1)).astype(np.uint32)


def links_of(slots, slot_offsets, first, n_records: int, window: int = DEFAULT_WINDOW, mate=None) -> np.ndarray:
    """int32 [n_records, window, 2]: link[t][k - 1][0] counts the reads with equal observations at t and t - k, [1] with unequal.
    ``mate`` (section 7i): the fragments are counted instead, a pair once over its ``fragment_observations``."""
    link = np.zeros((n_records, window, 2), np.int32)
    if mate is not None:
        slots, slot_offsets, first = fragment_observations(slots, slot_offsets, first, mate)
    for r in range(len(first)):
        if mate is not None and 0 <= mate[r] < r:
            continue                                    # the pair was counted at its first read
        s0, s1 = int(slot_offsets[r]), int(slot_offsets[r + 1])
        for s in range(s0, s1):
            if slots[s] < 0:
                continue
            for k in range(1, min(window, s - s0) + 1):
                if slots[s - k] >= 0:
                    link[int(first[r]) + s - s0, k - 1, int(slots[s] != slots[s - k])] += 1
    return link


def chain(link, window: int = DEFAULT_WINDOW, min_margin: int = DEFAULT_MIN_MARGIN, chromosome=None):
    """(set int32 [n], flip uint8 [n]): ``set[t]`` is the index of the record that opened the set of t."""
    link = np.asarray(link, np.int32).reshape(-1, window, 2)
    n = link.shape[0]
    chromosome = np.zeros(n, np.int32) if chromosome is None else np.asarray(chromosome, np.int32)
    sets, flip = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for t in range(n):
        seen: Dict[int, List[int]] = {}                 # insertion order: the order of k
        for k in range(1, window + 1):
            s = t - k
            if s < 0 or chromosome[s] != chromosome[t]:
                continue
            cis, trans = int(link[t, k - 1, 0]), int(link[t, k - 1, 1])
            if flip[s]:
                cis, trans = trans, cis
            acc = seen.setdefault(int(sets[s]), [0, 0])
            acc[0] += cis
            acc[1] += trans
        best, margin = None, -1
        for g, (same, opp) in seen.items():
            if abs(same - opp) > margin:                # a tie stays with the set of the smaller k
                best, margin = g, abs(same - opp)
        if best is not None and margin >= min_margin:
            sets[t], flip[t] = best, int(seen[best][1] > seen[best][0])
        else:
            sets[t], flip[t] = t, 0
    return sets, flip


def set_positions(sets, positions) -> np.ndarray:
    """int64 [n]: the POS of the first record of t's set, 0 when the set has one member (t is unphased)."""
    sets = np.asarray(sets, np.int64)
    positions = np.asarray(positions, np.int64)
    if sets.shape[0] == 0:
        return np.zeros(0, np.int64)
    members = np.bincount(sets, minlength=sets.shape[0])
    return np.where(members[sets] >= 2, positions[sets], 0).astype(np.int64)


def haplotags_of(slots, slot_offsets, first, sets, flip, positions, mate=None):
    """(hp uint8 [reads], ps int64 [reads]): a read's set is that of its first observation at a phased record; over its observations
    in that set, ``o xor flip`` counts into n1 / n2; hp 1, 2 or 0 (tie, or no set), ps the set's POS or 0.  ``mate`` (section 7i):
    the rule runs over the ``fragment_observations`` instead, so both mates of a pair get one tag."""
    if mate is not None:
        slots, slot_offsets, first = fragment_observations(slots, slot_offsets, first, mate)
    set_pos = set_positions(sets, positions)
    n = len(first)
    hp, ps = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    for r in range(n):
        s0, s1 = int(slot_offsets[r]), int(slot_offsets[r + 1])
        mine, count = None, [0, 0]
        for s in range(s0, s1):
            t = int(first[r]) + s - s0
            if slots[s] < 0 or set_pos[t] == 0:
                continue
            if mine is None:
                mine = int(sets[t])
                ps[r] = set_pos[t]
            if int(sets[t]) == mine:
                count[int(slots[s]) ^ int(flip[t])] += 1
        hp[r] = 1 if count[0] > count[1] else 2 if count[1] > count[0] else 0
    return hp, ps


def phased_line(line: bytes, rec: Record, flip: int, ps: int) -> bytes:
    """The line of a record in a set of at least two: GT ``a|b`` (``b|a`` when flipped), ``:PS`` behind FORMAT, ``:<ps>`` behind the
    sample column; nothing else changes."""
    body = line.rstrip(b"\r\n")
    f = body.split(b"\t")
    rest = f[9].split(b":", 1)
    gt = b"%d|%d" % ((rec.b, rec.a) if flip else (rec.a, rec.b))
    f[8] += b":PS"
    f[9] = b":".join([gt] + rest[1:]) + b":%d" % ps
    return b"\t".join(f) + line[len(body):]


def phased_header(header: str) -> str:
    """The header of the input with the PS declaration in front of the column line."""
    lines = header.splitlines(keepends=True)
    at = next((i for i, line in enumerate(lines) if line.startswith("#CHROM")), len(lines))
    return "".join(lines[:at]) + PS_HEADER + "".join(lines[at:])


# ------------------------------------------------------------------------------------------------
# the GPU
# ------------------------------------------------------------------------------------------------
_PROTOTYPES = (
    ("hello_phase_observe", READS + [i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, C.POINTER(vp)]),
    ("hello_phase_chain", [vp, vp, i64, i32, i32, vp, vp]),
    ("hello_phase_tag", [vp, vp, vp]),
    ("hello_phase_array", ARRAY_GETTER),
    ("hello_phase_stats", STATS_GETTER),
    ("hello_phase_fragments", [vp, vp, vp, vp, i64]),
    ("hello_phase_tag_fragments", [vp, vp, vp]),
    ("hello_phase_fragment_stats", STATS_GETTER),
    ("hello_phase_free", [vp], None),
)


def _lib():
    return bind(_PROTOTYPES)


class Phaser(Handle):
    """One chromosome's ``hello_phase`` handle: ``observe`` adds a batch of read sets, ``arrays`` gives the slots and the links so
    far, ``tag`` the haplotype of every read given, in the order given.  ``fragments`` (once, after the last ``observe``) joins
    the mates of all batches; ``arrays`` then holds ``mate`` and ``fragment_links`` too, and ``tag(..., fragments=True)`` tags both
    mates of a pair alike."""
    NAME, STAT_NAMES = "phase", STAT_NAMES

    def __init__(self, records: Sequence[Record], q_threshold: int = 10, mapq_threshold: int = 10, window: int = DEFAULT_WINDOW,
                 device: int = 0):
        self.n_records, self.window = len(records), int(window)
        self._starts = np.array([rec.start for rec in records], np.int64)
        self._ends = np.array([rec.end for rec in records], np.int64)
        text = [x for rec in records for x in (rec.allele_a, rec.allele_b)]
        self._alleles = np.frombuffer(b"".join(text), np.uint8)
        self._offsets = np.concatenate([[0], np.cumsum([len(x) for x in text])]).astype(np.int64)
        self._tail = (int(q_threshold), int(mapq_threshold), int(window), int(device))
        super().__init__(_lib())
        shape = (self.n_records, self.window, 2)
        self.ARRAYS = (("slots", SLOTS, np.int8, None), ("slot_offsets", SLOT_OFFSETS, np.int64, None), ("first", FIRST, np.int64, None),
                       ("links", LINKS, np.int32, shape), ("mate", MATE, np.int64, None), ("fragment_links", FRAGMENT_LINKS, np.int32, shape))
        self._joined = False

    def fragments(self, name_hash, flags, source) -> np.ndarray:
        """``hello_phase_fragments`` with name_hash / flags / source of every read observed, in the order given -> mate int64."""
        name_hash, flags = np.ascontiguousarray(name_hash, np.uint64), np.ascontiguousarray(flags, np.uint16)
        source = np.ascontiguousarray(source, np.uint8)
        if not name_hash.shape == flags.shape == source.shape or name_hash.ndim != 1:
            raise ValueError("name_hash, flags and source: one entry per read")
        check(self._lib.hello_phase_fragments(self._h, name_hash.ctypes.data, flags.ctypes.data, source.ctypes.data,
                                              int(name_hash.shape[0])))
        self._joined = True
        return self._array(MATE, np.int64)

    def fragment_stats(self) -> Dict[str, float]:
        return handle_stats(self._lib.hello_phase_fragment_stats, self._h, FRAGMENT_STAT_NAMES)

    def observe(self, reads: Sequence[Reads]) -> None:
        if not 1 <= len(reads) <= 2:
            raise ValueError("one or two read sets (BAM files)")
        r, source = Reads.concat(list(reads))
        ptr = lambda a: a.ctypes.data  # noqa: E731
        check(self._lib.hello_phase_observe(*r.pointers(source), int(r.n_reads), ptr(self._starts), ptr(self._ends),
                                            ptr(self._alleles), ptr(self._offsets), self.n_records, *self._tail, C.byref(self._h)))

    def _has(self, name: str) -> bool:
        return name not in ("mate", "fragment_links") or self._joined

    def tag(self, sets, flip, fragments: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        sets, flip = np.ascontiguousarray(sets, np.int32), np.ascontiguousarray(flip, np.uint8)
        if sets.shape != (self.n_records,) or flip.shape != (self.n_records,):
            raise ValueError("set and flip: one entry per record")
        tag = self._lib.hello_phase_tag_fragments if fragments else self._lib.hello_phase_tag
        check(tag(self._h, sets.ctypes.data, flip.ctypes.data))
        return self._array(HP, np.uint8), self._array(PS, np.int64)



def find_observations(reads: Sequence[Reads], records: Sequence[Record], q_threshold: int = 10, mapq_threshold: int = 10,
                      window: int = DEFAULT_WINDOW, device: int = 0):
    """One ``hello_phase_observe`` call over already decoded read sets (one per BAM, at most two) -> ({slots, slot_offsets, first,
    links}, statistics)."""
    with Phaser(records, q_threshold, mapq_threshold, window, device) as ph:
        ph.observe(reads)
        return ph.arrays(), ph.stats()


def chain_native(link, window: int = DEFAULT_WINDOW, min_margin: int = DEFAULT_MIN_MARGIN, chromosome=None):
    """``hello_phase_chain``: the chain on the host in C++ (no GPU) -> (set, flip)."""
    link = np.ascontiguousarray(link, np.int32).reshape(-1, window, 2)
    n = link.shape[0]
    chromosome = np.zeros(n, np.int32) if chromosome is None else np.ascontiguousarray(chromosome, np.int32)
    if chromosome.shape != (n,):
        raise ValueError("chromosome: one entry per record")
    sets, flip = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    lib = _lib()
    check(lib.hello_phase_chain(link.ctypes.data, chromosome.ctypes.data, n, int(window), int(min_margin), sets.ctypes.data,
                                flip.ctypes.data))
    return sets, flip


def find_haplotags(reads: Sequence[Reads], records: Sequence[Record], q_threshold: int = 10, mapq_threshold: int = 10,
                   window: int = DEFAULT_WINDOW, min_margin: int = DEFAULT_MIN_MARGIN, device: int = 0, details: Optional[dict] = None,
                   fragments: bool = False):
    """Observe, chain and tag in one go -> (hp uint8, ps int64), aligned with the reads of the sets one after the other.
    ``details``: filled with the arrays of ``find_observations``, ``set``, ``flip`` and ``stats``.  ``fragments`` (section 7i): the
    mates of a pair are joined, the chain runs on the fragment links and both mates get one tag; ``details`` also holds ``mate``,
    ``fragment_links`` and the fragment statistics."""
    with Phaser(records, q_threshold, mapq_threshold, window, device) as ph:
        ph.observe(reads)
        if fragments:
            rd, source = Reads.concat(list(reads))
            ph.fragments(rd.name_hash, rd.flags, source)
        got = ph.arrays()
        sets, flip = chain_native(got["fragment_links" if fragments else "links"], window, min_margin)
        hp, ps = ph.tag(sets, flip, fragments)
        if details is not None:
            details.update(got, set=sets, flip=flip, stats=dict(ph.stats(), **(ph.fragment_stats() if fragments else {})))
        return hp, ps


# ------------------------------------------------------------------------------------------------
# the file
# ------------------------------------------------------------------------------------------------
def read_vcf(path: str):
    """-> (header text, every other line's bytes in file order)."""
    header, lines = [], []
    with open(path, "rb") as fh:
        for line in fh:
            (header if line.startswith(b"#") and not lines else lines).append(line)
    return b"".join(header).decode(), lines


def _from(rd: Reads, lo: int) -> Reads:
    """The reads that start at or behind ``lo``: a read belongs to the span that holds its start."""
    keep = np.flatnonzero(rd.ref_starts >= lo)
    if keep.shape[0] == rd.n_reads:
        return rd

    def ragged(values, offsets):
        lens, begin = np.diff(offsets)[keep], offsets[:-1][keep]
        new = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return values[np.repeat(begin - new[:-1], lens) + np.arange(int(new[-1]))], new
    bases, read_offsets = ragged(rd.bases, rd.read_offsets)
    quals, _ = ragged(rd.quals, rd.read_offsets)
    cigars, cigar_offsets = ragged(rd.cigars, rd.cigar_offsets)
    return Reads(bases=bases, quals=quals, read_offsets=read_offsets, cigars=cigars, cigar_offsets=cigar_offsets,
                 ref_starts=rd.ref_starts[keep], ref_ends=rd.ref_ends[keep], mapq=rd.mapq[keep], flags=rd.flags[keep],
                 name_hash=rd.name_hash[keep], strand=rd.strand[keep], hp=rd.hp[keep])


def chromosome_phase(handles: Sequence[BamFile], chromosome: str, length: int, records: Sequence[Record], q_threshold: int = 10,
                     mapq_threshold: int = 10, window: int = DEFAULT_WINDOW, min_margin: int = DEFAULT_MIN_MARGIN, device: int = 0,
                     restatement: bool = False, max_span: Optional[int] = None, stats: Optional[dict] = None,
                     fragments: bool = False) -> Dict[str, np.ndarray]:
    """One chromosome: {slots, slot_offsets, first, links, set, flip, hp, ps}; the per-read arrays follow the reads of span after
    span, within a span the BAMs one after the other.  ``fragments`` (section 7i): the mates of a pair are joined across all
    spans -- ``mate`` and ``fragment_links`` are in the result, the chain runs on the fragment links and both mates get one tag."""
    step, n = span_step(max_span), len(records)
    positions = [rec.pos for rec in records]
    _check_sorted(records)
    add = adder(stats)
    ph = None if restatement else Phaser(records, q_threshold, mapq_threshold, window, device)
    try:
        parts, links = [], np.zeros((n, window, 2), np.int32)
        names, flags, sources, is_counted = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint16)], [np.zeros(0, np.uint8)], [np.zeros(0, bool)]
        for lo in range(0, length, step):
            t0 = time.perf_counter()
            sets = [_from(h.fetch(chromosome, lo, min(lo + step, length)), lo) for h in handles]
            t1 = time.perf_counter()
            if fragments:                               # what joins the mates, in the handle's read order
                for i, rd in enumerate(sets):
                    names.append(rd.name_hash)
                    flags.append(rd.flags)
                    sources.append(np.full(rd.n_reads, i, np.uint8))
                    if restatement:
                        is_counted.append(counted_mask(rd, mapq_threshold))
            if restatement:
                slots, offsets, first = slots_of(sets, records, q_threshold, mapq_threshold)
                links += links_of(slots, offsets, first, n, window)
                parts.append((slots, offsets, first))
            else:
                ph.observe(sets)
            add("decode_s", t1 - t0)
            add("observe_s", time.perf_counter() - t1)
            add("calls", 1)
        t0 = time.perf_counter()
        if restatement:
            offsets, base = [np.zeros(1, np.int64)], 0
            for _, o, _ in parts:
                offsets.append(o[1:] + base)
                base += int(o[-1])
            out = dict(slots=np.concatenate([p[0] for p in parts] or [np.zeros(0, np.int8)]), slot_offsets=np.concatenate(offsets),
                       first=np.concatenate([p[2] for p in parts] or [np.zeros(0, np.int64)]), links=links)
            mate = None
            if fragments:
                mate, counts = join_mates(np.concatenate(names), np.concatenate(flags), np.concatenate(sources),
                                          np.concatenate(is_counted))
                out.update(mate=mate, fragment_links=links_of(out["slots"], out["slot_offsets"], out["first"], n, window, mate))
                for k, v in counts.items():
                    add(k, v)
            out["set"], out["flip"] = chain(out["fragment_links"] if fragments else links, window, min_margin)
            add("chain_s", time.perf_counter() - t0)
            out["hp"], out["ps"] = haplotags_of(out["slots"], out["slot_offsets"], out["first"], out["set"], out["flip"], positions,
                                                mate)
        else:
            if fragments:
                ph.fragments(np.concatenate(names), np.concatenate(flags), np.concatenate(sources))
                add("join_s", time.perf_counter() - t0)
                t0 = time.perf_counter()
            out = ph.arrays()
            out["set"], out["flip"] = chain_native(out["fragment_links" if fragments else "links"], window, min_margin)
            add("chain_s", time.perf_counter() - t0)
            out["hp"], out["ps"] = ph.tag(out["set"], out["flip"], fragments)
            for k, v in dict(ph.stats(), **(ph.fragment_stats() if fragments else {})).items():
                add(k, v)
        return out
    finally:
        if ph is not None:
            ph.close()


def write_phased_vcf(vcf_path: str, bams: Sequence[str], out_path: str, chromosomes: Optional[Sequence[str]] = None,
                     q_threshold: int = 10, mapq_threshold: int = 10, window: int = DEFAULT_WINDOW,
                     min_margin: int = DEFAULT_MIN_MARGIN, device: int = 0, restatement: bool = False, max_span: Optional[int] = None,
                     stats: Optional[dict] = None, haplotags: Optional[dict] = None, fragments: bool = False) -> str:
    """``out_path``: the header of ``vcf_path`` with the PS declaration and its lines in its order, those of the records in a phase
    set of at least two rewritten by ``phased_line``.  Records of ``chromosomes`` (default: every chromosome of the file) are
    phased; chromosome lengths come from the BAM header.  ``restatement``: everything comes from the plain-Python rules instead of
    the GPU (what the tests compare the GPU's file with).  ``haplotags``: filled with {chromosome: (hp, ps)}.  ``fragments``
    (--phase_fragments, section 7i): the two mates of a read pair count as one fragment."""
    if not 1 <= len(bams) <= 2:
        raise ValueError("one BAM, or an Illumina and a PacBio BAM")
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"window: 1 to {MAX_WINDOW}")
    if min_margin < 1:
        raise ValueError("min_margin: at least 1")
    header, lines = read_vcf(vcf_path)
    by_chromosome: Dict[str, List[Tuple[int, Record]]] = {}
    for i, line in enumerate(lines):
        rec = phasable(line)
        c = line.split(b"\t", 1)[0].decode()
        if rec is not None and (not chromosomes or c in chromosomes):
            by_chromosome.setdefault(c, []).append((i, rec))
    handles = [BamFile(p) for p in bams]
    t_host = 0.0
    try:
        lengths = [dict(h.references) for h in handles]
        for c, recs in by_chromosome.items():
            if any(c not in known for known in lengths):
                raise ValueError(f"no sequence named {c!r} in the BAM header")
            records = [rec for _, rec in recs]
            got = chromosome_phase(handles, c, min(known[c] for known in lengths), records, q_threshold, mapq_threshold, window,
                                   min_margin, device, restatement, max_span, stats, fragments)
            t0 = time.perf_counter()
            set_pos = set_positions(got["set"], [rec.pos for rec in records])
            for (i, rec), flip, ps in zip(recs, got["flip"].tolist(), set_pos.tolist()):
                if ps:
                    lines[i] = phased_line(lines[i], rec, flip, ps)
            t_host += time.perf_counter() - t0
            if haplotags is not None:
                haplotags[c] = (got["hp"], got["ps"])
            _log.info("chromosome %s: %d phasable records, %d in %d phase sets", c, len(records), int((set_pos > 0).sum()),
                      len(set(set_pos[set_pos > 0].tolist())))
        t0 = time.perf_counter()
        with open(out_path, "wb") as out:
            out.write(phased_header(header).encode("ascii"))
            out.writelines(lines)
        t_host += time.perf_counter() - t0
    finally:
        for h in handles:
            h.close()
    if stats is not None:
        stats["write_s"] = stats.get("write_s", 0.0) + t_host
    return out_path


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Write a read-backed phased VCF from a VCF that already exists and the BAM(s) it was called from")
    p.add_argument("--vcf", required=True, help="The VCF whose heterozygous records are phased (results.output.vcf)")
    p.add_argument("--bam", required=True, help="The BAM, or Illumina,PacBio")
    p.add_argument("--output", required=True, help="Path of the phased VCF")
    p.add_argument("--chromosomes", help="Comma-separated chromosomes to phase (default: every chromosome of the VCF)")
    p.add_argument("--q_threshold", type=int, default=10, help="Base quality threshold")
    p.add_argument("--mapq_threshold", type=int, default=10, help="Mapping quality threshold")
    p.add_argument("--phase_window", type=int, default=DEFAULT_WINDOW, help="Records back that a record is linked to (1 to 32)")
    p.add_argument("--phase_min_margin", type=int, default=DEFAULT_MIN_MARGIN, help="Smallest |cis - trans| that joins a set")
    p.add_argument("--phase_fragments", action="store_true", default=False,
                   help="The two mates of a read pair act as one fragment: joined by name on the GPU, linked and tagged together")
    p.add_argument("--device", type=int, default=0, help="GPU index")
    return p


def main(argv=None) -> str:
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)-15s %(message)s")
    if not 1 <= args.phase_window <= MAX_WINDOW:
        raise SystemExit(f"--phase_window: 1 to {MAX_WINDOW}")
    if args.phase_min_margin < 1:
        raise SystemExit("--phase_min_margin: at least 1")
    bams = args.bam.split(",")
    if len(bams) > 2:
        raise SystemExit("--bam takes one or two files")
    return write_phased_vcf(args.vcf, bams, args.output, args.chromosomes.split(",") if args.chromosomes else None, args.q_threshold,
                            args.mapq_threshold, args.phase_window, args.phase_min_margin, args.device, fragments=args.phase_fragments)


if __name__ == "__main__":
    main(sys.argv[1:])
