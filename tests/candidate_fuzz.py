"""The fuzz corpus of tests/read_fuzz.py for the stages that decide every call: the hotspot detector (7b) and
the candidate stage (7c) of one Illumina BAM, one PacBio BAM and both together.

``padded(seed, profile)`` sets a corpus inside random bases, so that the reference's window rule skips no chunk; ``inputs(seed,
route, pad)`` are the read rows per BAM of a route, with the reads ``additions`` builds on purpose appended; ``restated`` runs the
three restatements (tests/hotspot_reference.py, candidate_reference.py, pacbio_reference.py, hybrid_reference.py) on them.
``Oracle`` derives the counting layer, the strict clip, the allele records and the sites from ``read_fuzz.alignment_table`` with
NumPy group-bys and string joins -- no cursor walks a CIGAR there -- and ``Rules`` switches each rule off.  ``survey`` counts what
tests/test_candidate_fuzz.py asserts; ``hand_built`` is the read set of the census lines no corpus reaches.
"""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass
from typing import Dict, List, Sequence, Set, Tuple

import numpy as np

from tests import candidate_reference as cr
from tests import hotspot_reference as hr
from tests import hybrid_reference as hy
from tests import pacbio_reference as pr
from tests import qc_cases, read_fuzz as rf
from tests.gvcf_cases import D, EQ, H, I, M, N, P, S, X

K_TILE = 256                                  # kTile of differing.h
PAD_LEFT = K_TILE                             # a multiple of the tile: the read fuzz's planted edges keep their phase
PAD_RIGHT = 2048                              # >= 1 600; the longest reference span of a read of the corpus is 1 858 (seed 11, long)
START = 16                                    # detection runs over [START, len)
LENGTH = PAD_LEFT + rf.LENGTH + PAD_RIGHT     # 4 904
SEEDS = rf.SEEDS
ROUTES = ("illumina", "pacbio", "two_bams", "hybrid")
PILE_SEED = 0                                 # the one corpus per route that holds the reads of the caps
DEEP_SEEDS = range(5)                         # the corpora with reads deep enough to open the two-BAM route's coverage gate
Q_THRESHOLD = MAPQ_THRESHOLD = 10
FEATURE_LENGTH = 150
REASSEMBLY_SIZE = 10
REV = rf.REV


def profiles_of(route: str) -> Tuple[str, ...]:
    return {"illumina": ("short",), "pacbio": ("long",)}.get(route, ("short", "long"))


# ------------------------------------------------------------------------------------------------
# the corpus layer
# ------------------------------------------------------------------------------------------------
def _pads(seed: int) -> Tuple[str, str]:
    """The random bases in front of and behind the corpus of ``seed``: the same for both profiles, so two BAMs share them."""
    rng = np.random.default_rng([seed, 20261021])
    return "".join(rng.choice(list("ACGT"), size=PAD_LEFT)), "".join(rng.choice(list("ACGT"), size=PAD_RIGHT))


@functools.lru_cache(maxsize=None)
def padded(seed: int, profile: str, keep_case: bool = False, reference_of: str = None):
    """-> (reference, rows, records): the corpus with its reference upper-cased (or with case kept) inside PAD_LEFT random ACGT
    bases in front and PAD_RIGHT behind; read and record positions are shifted."""
    reference, rows, records = rf.corpus(seed, profile, reference_of=reference_of)
    left, right = _pads(seed)
    reference = left + (reference if keep_case else reference.upper()) + right
    rows = [r[:2] + (r[2] + PAD_LEFT,) + r[3:] for r in rows]
    return reference, rows, [rec._replace(start=rec.start + PAD_LEFT, end=rec.end + PAD_LEFT) for rec in records]


def _row(name: int, pos: int, cigar, bases: str, flag: int = 0, quality: int = 30, mapq: int = 60) -> tuple:
    assert len(bases) == sum(n for op, n in cigar if op in (M, I, S, EQ, X))
    return (name, flag, pos, list(cigar), bases, [quality] * len(bases), mapq)


EVENTS = (("D", 78), ("D", 79), ("DD", 79), ("D", 99), ("D", 100), ("D", 101), ("I", 77), ("I", 78), ("I", 79), ("I", 80), ("I", 99), ("I", 100),
          ("I", 101))
EVENT_SLOTS = tuple(PAD_LEFT + rf.LENGTH + k for k in (1000, 1330, 1660))    # where the three events of a corpus begin


def _event_rows(rng, reference: str, kind: str, n: int, at: int, name: int, carriers: int = 6) -> List[tuple]:
    """``carriers`` reads that carry one event of ``n`` bases behind 30 aligned bases from ``at`` on, and as many that carry the
    reference; "DD": two deletions of ``n`` 41 bases apart, the second location meets an empty cluster (cluster_locations)."""
    out = []
    flank = 30
    for k in range(2 * carriers):
        flag = REV * (k & 1)
        if k >= carriers:                                                # the reference's haplotype
            span = 2 * flank + (n if kind == "D" else 0) + (2 * n + 41 if kind == "DD" else 0)
            out.append(_row(name + k, at, [(M, span)], reference[at:at + span], flag))
        elif kind == "I":
            text = "".join(rng.choice(list("ACGT"), size=n)) if k == 0 else out[0][4][flank:flank + n]
            out.append(_row(name + k, at, [(M, flank), (I, n), (M, flank)], reference[at:at + flank] + text + reference[at + flank:at + 2 * flank], flag))
        elif kind == "D":
            out.append(_row(name + k, at, [(M, flank), (D, n), (M, flank)], reference[at:at + flank] + reference[at + flank + n:at + 2 * flank + n], flag))
        else:
            b = at + flank + n
            out.append(_row(name + k, at, [(M, flank), (D, n), (M, 41), (D, n), (M, flank)],
                            reference[at:at + flank] + reference[b:b + 41] + reference[b + 41 + n:b + 41 + n + flank], flag))
    return out


def _partial_rows(rng, reference: str, records, name: int) -> List[tuple]:
    """Around up to three planted insertion records: four carriers of the record's inserted text behind its anchor (made at least
    three bases long by bases in front of it), a read whose first operation is an ``I`` with a proper suffix of that text, one whose
    last operation is an ``I`` with a proper prefix, a pair whose suffix and prefix match no key; at every other record four
    carriers of a second key that shares the suffix, and of a third that shares the prefix: such a partial joins nothing."""
    out = []
    chosen = [rec for rec in records if rec.end - rec.start == 1 and max(len(rec.allele_a), len(rec.allele_b)) > 1
              and START + 60 < rec.start < LENGTH - 60 and set(reference[rec.start - 30:rec.start + 31]) <= set("ACGT")][:6:2]
    for k, rec in enumerate(chosen):
        p = rec.start
        own = max(rec.allele_a, rec.allele_b, key=len).decode()[1:]
        text = ("GA" + own)[-max(3, len(own)):] if len(own) < 3 else own
        keys = [text]
        if k % 2 == 1:
            keys += [rf._other(rng, text[0]) + text[1:], text[:-1] + rf._other(rng, text[-1])]
        left, right = reference[p - 24:p + 1], reference[p + 1:p + 26]
        for key in keys:
            for j in range(4):
                out.append(_row(name + len(out), p - 24, [(M, 25), (I, len(key)), (M, 25)], left + key + right, REV * (j & 1)))
        for j in range(3):                                                # reference reads, so that the totals are not the carriers' alone
            out.append(_row(name + len(out), p - 24, [(M, 50)], reference[p - 24:p + 26], REV * (j & 1)))
        out.append(_row(name + len(out), p + 1, [(I, len(text) - 1), (M, 25)], text[1:] + right))                     # suffix
        out.append(_row(name + len(out), p - 24, [(M, 25), (I, len(text) - 1)], left + text[:-1]))                    # prefix
        wrong = rf._other(rng, text[-1]) + rf._other(rng, text[0])
        out.append(_row(name + len(out), p + 1, [(I, 2), (M, 25)], wrong + right))                                     # no key ends so
        out.append(_row(name + len(out), p - 24, [(M, 25), (I, 2)], left + wrong[::-1]))                          # none begins so
    return out


def _pile_rows(reference: str, at: int, name: int, n: int) -> List[tuple]:
    """``n`` reads of 40 bases over one SNV at ``at``: every fifth carries it.  1 001 pass the Illumina cap of the cluster's 30-base
    fetch (1 000), the PacBio cap of that fetch (100), of pass 1's 180-base fetch (180) and of a hotspot chunk (1 000)."""
    ref = reference[at - 20:at + 20]
    alt = ref[:20] + "ACGT"[("ACGT".index(ref[20]) + 1) % 4] + ref[21:]
    return [_row(name + k, at - 20, [(M, 40)], alt if k % 5 == 0 else ref, REV * (k & 1)) for k in range(n)]


def _clip_rows(rng, reference: str, at: int, name: int) -> List[tuple]:
    """Long reads over one SNV at ``at``, built for the strict clip of the pass-2 fetch [at - 15, at + 15) of a lone site there.
    The flank's cut (the 201st read base counted outwards from the bound) falls on the first, a middle and the last base of an
    ``=``, ``X``, ``I`` and ``S``, inside an ``M``, and directly in front of, one and two bases behind a ``D``, an ``N`` and an
    ``I P I`` (the outermost kept operation is then an ``I`` and becomes ``S``); the bound itself falls on the first, the middle
    and the last base of an ``=``, ``X``, ``D`` and ``N`` (on the last the two halves' centre operations do not merge).  Each
    once for the left and once for the right bound.  Every third read carries the SNV."""
    lo, hi = at - 15, at + 15
    halves = [[(M, 300)]]                                                # outermost first, the inner M run last
    for j in (0, 2, 4):
        halves += [[(M, 40), (op, 5), (M, 200 - j)] for op in (EQ, X, I)]
        halves += [[(M, 40), (op, 5), (M, 201 - j // 2)] for op in (D, N)]
        halves += [[(M, 40), (I, 2), (P, 5), (I, 2), (M, 199 - j // 2)], [(H, 3), (S, 45), (M, 200 - 11 * j)]]
    reads = []
    for half in halves:
        span = sum(k for o, k in half if o in (M, D, N, EQ, X))
        reads.append((half + [(M, 260)], lo + 1 - span))                # the inner run ends on the left bound
        reads.append(([(M, 260)] + half[::-1], hi + 1 - 260))           # ... begins behind the right bound
    for op in (EQ, X, D, N):
        for j in (0, 2, 4):
            reads.append(([(M, 230), (op, 5), (M, 300)], lo - j - 230))
            reads.append(([(M, 300), (op, 5), (M, 230)], hi - j - 300))
    out = []
    for cigar, pos in reads:
        merged: List[Tuple[int, int]] = []
        for o, k in cigar:
            if merged and merged[-1][0] == o:
                merged[-1] = (o, merged[-1][1] + k)
            else:
                merged.append((o, k))
        bases, p = [], pos
        for o, k in merged:
            if o in (M, EQ, X):
                bases.append(reference[p:p + k])
            elif o in (I, S):
                bases.append("".join(rng.choice(list("ACGT"), size=k)))
            p += k if o in (M, D, N, EQ, X) else 0
        text = "".join(bases)
        i = _query_index(merged, pos, at)
        if len(out) % 3 == 0 and i >= 0:
            text = text[:i] + "ACGT"[("ACGT".index(reference[at]) + 1) % 4] + text[i + 1:]
        out.append(_row(name + len(out), pos, merged, text, REV * (len(out) & 1)))
    return out


def _query_index(cigar, pos: int, at: int) -> int:
    """The read base aligned at reference position ``at``, or -1 (generator's helper: the tests' quantities do not use it)."""
    q, p = 0, pos
    for o, k in cigar:
        if o in (M, EQ, X) and p <= at < p + k:
            return q + at - p
        q += k if o in (M, I, S, EQ, X) else 0
        p += k if o in (M, D, N, EQ, X) else 0
    return -1


def _deep_rows(reference: str, at: int, name: int, snvs: int) -> List[tuple]:
    """Forty reads of 60 bases over ``snvs`` SNVs three bases apart, every fourth read carrying them all: the coverage gate of the
    two-BAM route opens (40 > 14).  Ten SNVs are a cluster of ten regions, which is then not reassembled
    (``clusters_skipped_for_size``); one SNV is reassembled and its PacBio reads are reassigned."""
    ref = reference[at - 30:at + 30]
    alt = list(ref)
    for k in range(snvs):
        alt[16 + 3 * k] = "ACGT"[("ACGT".index(ref[16 + 3 * k]) + 1) % 4]
    return [_row(name + k, at - 30, [(M, 60)], "".join(alt) if k % 4 == 0 else ref, REV * (k & 1)) for k in range(40)]


def _skip_rows(reference: str, at: int, name: int) -> List[tuple]:
    """Sixteen reads over one SNV at ``at``, two of which carry it (2 / 16 = 0.125 >= 0.12), and one read whose ``N`` spans it:
    counted there it would make 2 / 17 < 0.12."""
    ref = reference[at - 20:at + 20]
    alt = ref[:20] + "ACGT"[("ACGT".index(ref[20]) + 1) % 4] + ref[21:]
    out = [_row(name + k, at - 20, [(M, 40)], alt if k < 2 else ref, REV * (k & 1)) for k in range(16)]
    return out + [_row(name + 16, at - 30, [(M, 20), (N, 30), (M, 20)], reference[at - 30:at - 10] + reference[at + 20:at + 40])]


def _lead_rows(rng, reference: str, at: int, name: int) -> List[tuple]:
    """The same sixteen reads over an SNV at ``at``, and one read that begins behind it with an ``I`` as operation 0: the
    insertion is planted at ``at``, where ``total += 1`` makes 2 / 17."""
    out = _skip_rows(reference, at, name)[:16]
    return out + [_row(name + 16, at + 1, [(I, 3), (M, 30)], "".join(rng.choice(list("ACGT"), size=3)) + reference[at + 1:at + 31])]


def _anchor_rows(reference: str, at: int, name: int) -> List[tuple]:
    """Four reads that begin behind ``at`` with ``5S 4D``, the last soft-clipped base an A, C, G and T in turn, and eight reads
    of the reference: four keys (ref, that base) of one read each stay below the count an indel needs; were the anchor not the
    soft-clipped base they would be one key of four reads."""
    out = [_row(name + k, at - 20, [(M, 45)], reference[at - 20:at + 25], REV * (k & 1)) for k in range(8)]
    return out + [_row(name + 8 + k, at + 1, [(S, 5), (D, 4), (M, 30)], "GGTC" + b + reference[at + 5:at + 35]) for k, b in enumerate("ACGT")]


@functools.lru_cache(maxsize=None)
def additions(seed: int, profile: str, reference_of: str = None) -> List[tuple]:
    """The reads built on purpose for the padded corpus (seed, profile): what the grammar reaches too rarely.
    They are appended to the corpus, never drawn from its generator's stream."""
    reference, rows, records = padded(seed, profile, reference_of=reference_of)
    rng = np.random.default_rng([seed, rf.PROFILES.index(profile), 20261022])
    name = 100000 * (1 + rf.PROFILES.index(profile))
    out: List[tuple] = []
    for slot, at in enumerate(EVENT_SLOTS):
        kind, n = EVENTS[(3 * seed + slot + rf.PROFILES.index(profile)) % len(EVENTS)]
        out += _event_rows(rng, reference, kind, n, at, name + len(out))
    out += _partial_rows(rng, reference, records, name + len(out))
    twice = out[0]                                                      # the same (name, strand) twice: the second is dropped
    out.append(twice[:2] + (twice[2] + 3,) + twice[3:])
    out += _anchor_rows(reference, PAD_LEFT + rf.LENGTH + 780, name + len(out))
    out += _skip_rows(reference, PAD_LEFT + rf.LENGTH + 850, name + len(out))
    out += _lead_rows(rng, reference, PAD_LEFT + rf.LENGTH + 920, name + len(out))
    if seed == PILE_SEED:
        out += _pile_rows(reference, PAD_LEFT + rf.LENGTH + 700, name + len(out), 1001)
    if seed in DEEP_SEEDS:
        out += _deep_rows(reference, PAD_LEFT + rf.LENGTH + 1960, name + len(out), 10)
        out += _deep_rows(reference, 130, name + len(out), 1)
    if profile == "long":
        out += _clip_rows(rng, reference, PAD_LEFT + rf.LENGTH + 400, name + len(out))
    return out


@functools.lru_cache(maxsize=None)
def inputs(seed: int, route: str, pad: bool = True, keep_case: bool = False, extra: bool = True):
    """-> (reference, [rows of the route's BAMs, as a BAM holds them, sorted by position]).  ``pad`` False: the corpus as it stands,
    on its 2 600 bases, where chunks, regions and clusters leave the chromosome.  In the two-BAM routes the long reads are those
    drawn on the short corpus's chromosome (``reference_of``)."""
    sets = []
    for profile in profiles_of(route):
        of = "short" if len(profiles_of(route)) == 2 and profile == "long" else None
        if pad:
            reference, rows, _ = padded(seed, profile, keep_case, of)
            rows = rows + (additions(seed, profile, of) if extra else [])
        else:
            reference, rows, _ = rf.corpus(seed, profile, reference_of=of)
            reference = reference if keep_case else reference.upper()
        sets.append(sorted(rf.bam_rows(rows), key=lambda r: r[2]))       # stable: the corpus's order among equal positions
    return reference, sets


def span_of(reference: str, pad: bool) -> Tuple[int, int]:
    return (START if pad else 0), len(reference)


def reads_of(rows):
    return rf.bam_reads(rows)


def read_set(rows):
    return qc_cases.read_set(rows)


# ------------------------------------------------------------------------------------------------
# the restatements on one input
# ------------------------------------------------------------------------------------------------
HOTSPOT_STATS = ("chunks", "chunks_without_reads", "chunks_out_of_bounds", "chunks_at_read_cap", "reads_counted", "tiles", "event_capacity")


def hotspot_plan(read_sets: Sequence[Sequence], reference: str, start: int, stop: int, pacbio: bool) -> Dict[str, int]:
    """The statistics of the hotspot stage's chunk plan, from ``hotspot_reference.chunk_reads`` and the window rule of
    ``do_chunk``; ``tiles`` and ``event_capacity`` as hotspots.hip defines them: a chunk's counted reads span [min start - 1, max
    end) in tiles of K_TILE, and every ``I`` and ``D`` operation of a counted read is one event of its chunk."""
    two = len(read_sets) == 2
    size = hr.CHUNK_SIZE_PACBIO if (two or pacbio) else hr.CHUNK_SIZE_ILLUMINA
    caps = (hr.MAX_NUM_READS_ILLUMINA, hr.MAX_NUM_READS_PACBIO) if two else ((hr.MAX_NUM_READS_PACBIO,) if pacbio else (hr.MAX_NUM_READS_ILLUMINA,))
    st = dict.fromkeys(HOTSPOT_STATS, 0)
    for b in range(start, stop, size):
        e = min(b + size, stop)
        st["chunks"] += 1
        kept = [hr.chunk_reads(reads, b, e, cap) for reads, cap in zip(read_sets, caps)]
        reads = [r for k, _ in kept for r in k]
        if not reads:
            st["chunks_without_reads"] += 1
        elif min([r.pos for r in reads] + [b]) - 10 < 0 or max(r.ref_end for r in reads) > len(reference):
            st["chunks_out_of_bounds"] += 1
        else:
            st["chunks_at_read_cap"] += int(any(c for _, c in kept))
            counted = [r for r in reads if r.mapq >= MAPQ_THRESHOLD]
            st["reads_counted"] += len(counted)
            if counted:
                st["tiles"] += -(-(max(r.ref_end for r in counted) - min(r.pos for r in counted) + 1) // K_TILE)
                st["event_capacity"] += sum(op in (I, D) for r in counted for op, _ in r.cigar)
    return st


@functools.lru_cache(maxsize=None)
def restated(seed: int, route: str, pad: bool = True, extra: bool = True) -> Dict[str, object]:
    """The restatements on ``inputs(seed, route, pad)``: the hotspot positions (``hotspots``) and plan statistics, and from
    ``positions`` the sites with their statistics (``regions_pass1`` / ``regions_pass2`` among them) and, per technology, the
    gathered reads as indices into the input (``read_index``; the PacBio restatement keeps no way back from a clipped copy).
    ``positions`` are the hotspots; where the unpadded input has none -- its one 10 000-base chunk begins at 0 and is skipped -- the
    padded input's hotspots on the corpus's own 2 600 bases, shifted back."""
    reference, sets = inputs(seed, route, pad, extra=extra)
    reads = [reads_of(rows) for rows in sets]
    start, stop = span_of(reference, pad)
    pacbio, hybrid = route == "pacbio", route == "hybrid"
    plan = hotspot_plan(reads, reference, start, stop, pacbio)
    hotspots = hr.find_hotspots(reads, reference, start, stop, pacbio=pacbio, hybrid_hotspot=hybrid, q_threshold=Q_THRESHOLD,
                                mapq_threshold=MAPQ_THRESHOLD)
    positions = hotspots
    if not pad and not hotspots:
        positions = [p - PAD_LEFT for p in restated(seed, route, True)["hotspots"] if PAD_LEFT <= p < PAD_LEFT + rf.LENGTH]
    st: Dict[str, object] = {}
    # hello_candidates_find refuses a PacBio read without a CIGAR operation on the reference (there is nothing to clip): the
    # candidate stage gets the PacBio rows without the corpus's one such read, the hotspot stage gets them all
    site_rows = [rows if profile == "short" else [r for r in rows if r[3]] for rows, profile in zip(sets, profiles_of(route))]
    reads = [reads_of(rows) for rows in site_rows]
    if route == "illumina":
        sites = cr.find_candidates(reads[0], reference, positions, Q_THRESHOLD, MAPQ_THRESHOLD, FEATURE_LENGTH, st)
    elif route == "pacbio":
        sites = pr.find_candidates(reads[0], reference, positions, Q_THRESHOLD, MAPQ_THRESHOLD, FEATURE_LENGTH, st)
    else:
        sites = hy.find_candidates(reads[0], reads[1], reference, positions, hybrid, REASSEMBLY_SIZE, Q_THRESHOLD, MAPQ_THRESHOLD,
                                   FEATURE_LENGTH, st)
    where = [{id(r): i for i, r in enumerate(rs)} for rs in reads]
    if route == "illumina":
        index = [[where[0][id(s.reads[i])] for s in sites for _, idx in s.alleles for i in idx]]
    elif route == "pacbio":
        index = []
    else:
        index = [[where[0][id(s.reads0[i])] for s in sites for _, i0, _ in s.alleles for i in i0],
                 [where[1][id(s.originals1[i])] for s in sites for _, _, i1 in s.alleles for i in i1]]
    return dict(reference=reference, rows=sets, site_rows=site_rows, reads=reads, hotspots=hotspots, positions=positions, sites=sites, stats=st,
                read_index=index, plan=plan)


def stat_keys(route: str) -> Tuple[str, ...]:
    return hy.STAT_KEYS if len(profiles_of(route)) == 2 else cr.STAT_KEYS


def candidate_sites(route: str, sites, chromosome: str = "chr"):
    return (hy if len(profiles_of(route)) == 2 else cr).candidate_sites(sites, chromosome)


# ------------------------------------------------------------------------------------------------
# the oracle: everything from the alignment table, no cursor walks a CIGAR
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rules:
    """Every counting, record and site rule of sections 7b and 7c the oracle knows, each of which can be switched off."""
    eqx_counted: bool = True                 # = and X count as M
    n_uncounted: bool = True                 # N advances the reference without counting
    lead_total: bool = True                  # total += 1 at the planting position of an insertion that is operation 0
    increment_2: bool = True                 # an Illumina indel counts 2, a PacBio one 1
    softclip_anchor: bool = True             # a deletion's alt is the read base before it, a soft-clipped one too
    ph_keep_index: bool = True               # P and H are operations: an I behind a leading H is not operation 0
    single_inclusive: bool = True            # single flagging: an indel flags pos ... pos + |ref| inclusive
    hybrid_exclusive: bool = True            # hybrid flagging: pos ... pos + |ref| exclusive
    limit_100: bool = True                   # single flagging skips a key whose ref or alt is longer than 100
    mapq_by_caller: bool = True              # a read below the mapq threshold is selected (window, cap, names) but not counted
    qc_fail_kept: bool = True                # 0x200 does not make a read unusable
    improper_dropped: bool = True            # a paired read that is no proper pair is unusable
    first_of_name: bool = True               # only the first read of each (name, strand) is kept
    del_q60: bool = True                     # a deleted position has quality 60
    n_dropped_from_candidates: bool = True   # an allele with N is no candidate, but it keeps its supporting reads
    limit_80: bool = True                    # alleles above 80 bases are dropped; cluster_locations' quirk at 80
    strict_drop: bool = True                 # a flagged run that leaves [start, stop] is dropped whole, not cut


class Lines:
    """``read_fuzz.alignment_table`` of one BAM's rows with base and quality per line, and the per-read quantities that need no
    walk: the end as the start plus the number of lines with a reference position (at least one)."""

    def __init__(self, rows):
        t = rf.alignment_table(rows)
        self.rows, self.n = rows, len(rows)
        self.read, self.opi, self.q, self.p, self.op = t.read, t.opi, t.q, t.p, t.op
        length = np.array([len(r[4]) for r in rows], np.int64)
        off = np.cumsum(length) - length
        bases = np.frombuffer("".join(r[4] for r in rows).encode(), np.uint8)
        quals = np.array([v for r in rows for v in r[5]], np.int64)
        has_q = self.q >= 0
        at = np.where(has_q, off[self.read] + self.q, 0) if self.read.size else self.q
        self.base = np.where(has_q, bases[at], 0).astype(np.uint8) if bases.size else np.zeros(self.q.shape[0], np.uint8)
        self.qual = np.where(has_q, quals[at], 0) if quals.size else np.zeros(self.q.shape[0], np.int64)
        self.name = np.array([r[0] for r in rows], np.int64)
        self.flag = np.array([r[1] for r in rows], np.int64)
        self.pos = np.array([r[2] for r in rows], np.int64)
        self.mapq = np.array([r[6] for r in rows], np.int64)
        self.end = self.pos + np.maximum(np.bincount(self.read[self.p >= 0], minlength=self.n), 1)
        self.first = np.searchsorted(self.read, np.arange(self.n), "left")
        self.count = np.bincount(self.read, minlength=self.n)


@dataclass
class Sub:
    """The lines of the reads one searcher keeps (``r``: index into ``reads``, the reads' indices in the BAM), after the clip."""
    tech: int
    reads: np.ndarray
    capped: bool
    r: np.ndarray
    opi: np.ndarray
    op: np.ndarray
    p: np.ndarray
    base: np.ndarray
    qual: np.ndarray
    pos: np.ndarray            # per read, after the clip
    end: np.ndarray
    mapq: np.ndarray
    cut: list                  # (read, side, operation of the flank's cut line, of the bound's line, placement) per clip


_QUERY = np.isin(np.arange(16), (M, I, S, EQ, X))
FLANK = 200                    # strictClipRead's flank: 201 read bases are kept from the bound outwards


class Oracle:
    def __init__(self, reference: str, sets: Sequence[Sequence[tuple]], pacbio: bool = False, hybrid_hotspot: bool = False,
                 rules: Rules = Rules()):
        self.reference, self.rules, self.hybrid = reference, rules, hybrid_hotspot
        self.ref = np.frombuffer(reference.encode(), np.uint8)
        self.lines = [Lines(rows) for rows in sets]
        self.tech = [1] if pacbio else list(range(len(sets)))
        self.two = len(sets) == 2
        self.census: Counter = Counter()
        self.planted: List[int] = []             # the planting positions of the events of the last ``count``
        self.tiles: List[np.ndarray] = []        # per chunk of the last ``hotspots``: the events per tile of K_TILE positions

    # ---- selection -------------------------------------------------------------------------------
    def select(self, k: int, lo: int, hi: int, cap: float) -> Tuple[np.ndarray, bool]:
        """The reads of BAM ``k`` a searcher over [lo, hi) keeps under ``cap``, in file order, and whether the cap cut some."""
        L, r = self.lines[k], self.rules
        f = L.flag
        ok = (f & (0x4 | 0x100 | 0x800 | 0x400)) == 0
        ok &= ((f & 0x200) == 0) | r.qc_fail_kept
        ok &= ((f & 1) == 0) | ((f & 2) != 0) | (not r.improper_dropped)
        ok &= (L.mapq > 0) & (L.pos < hi) & (L.end > lo)
        if not r.mapq_by_caller:
            ok &= L.mapq >= MAPQ_THRESHOLD
        idx = np.flatnonzero(ok)
        if r.first_of_name and idx.size:
            _, first = np.unique(L.name[idx] * 2 + ((f[idx] & REV) != 0), return_index=True)
            idx = idx[np.sort(first)]
        keep = int(np.ceil(cap))
        return idx[:keep], idx.size > keep

    def sub(self, k: int, reads: np.ndarray, capped: bool, lo: int, hi: int) -> Sub:
        L = self.lines[k]
        at = np.concatenate([np.arange(L.first[i], L.first[i] + L.count[i]) for i in reads] + [np.zeros(0, np.int64)]).astype(np.int64)
        r = np.searchsorted(reads, L.read[at]) if at.size else at
        s = Sub(self.tech[k], reads, capped, r, L.opi[at].copy(), L.op[at].copy(), L.p[at].copy(), L.base[at].copy(), L.qual[at].copy(),
                L.pos[reads].copy(), L.end[reads].copy(), L.mapq[reads], [])
        if self.tech[k] == 1:
            self.clip(s, lo, hi)
        return s

    # ---- the strict clip -------------------------------------------------------------------------
    def clip(self, s: Sub, lo: int, hi: int) -> None:
        """python/PileupContainerLite.py strictClipRead on lines: a read that covers the bound keeps, from the bound's line
        outwards, the lines up to its 201st read base; an outermost kept ``I`` run becomes ``S``.  First the left bound ``lo``
        (the bound's own line belongs to the outer half), then ``hi`` (it belongs to the inner half)."""
        for side, bound in ((0, lo), (1, hi)):
            n = s.r.shape[0]
            if n == 0:
                return
            idx = np.arange(n)
            isq = _QUERY[s.op]
            cum = np.cumsum(isq)
            split = np.full(s.reads.shape[0], -1, np.int64)
            on = np.flatnonzero(s.p == bound)
            split[s.r[on]] = on
            sp = split[s.r]
            if side == 0:
                half = (sp >= 0) & (idx <= sp)
                a = cum[np.maximum(sp, 0)] - cum + isq
            else:
                half = (sp >= 0) & (idx > sp)
                a = cum - cum[np.maximum(sp, 0)]
            applies = np.zeros(s.reads.shape[0], bool)
            applies[s.r[half]] = True                                    # the right half may be empty: then nothing happens
            keep = ~(half & (a > FLANK + isq))
            lo_of, hi_of = np.searchsorted(s.r, np.arange(s.reads.shape[0]), "left"), np.searchsorted(s.r, np.arange(s.reads.shape[0]), "right")
            for rd in np.flatnonzero(applies):                           # the census of clip points
                mine = lo_of[rd] + np.flatnonzero(half[lo_of[rd]:hi_of[rd]])
                lost = mine[~keep[mine]]
                cutline = (lost[-1] + 1 if side == 0 else lost[0] - 1) if lost.size else -1
                if lost.size:
                    run = lo_of[rd] + np.flatnonzero(s.opi[lo_of[rd]:hi_of[rd]] == s.opi[cutline])
                    where = "whole" if not np.isin(run, lost).any() else "inside"
                    edge = "first" if cutline == run[0] else "last" if cutline == run[-1] else "middle"
                    s.cut.append((int(rd), side, int(s.op[cutline]), int(s.op[lost[-1] if side == 0 else lost[0]]), where, edge))
                    s.cut.append((int(rd), side, int(s.op[lost[-1] if side == 0 else lost[0]]), -1, "lost", ""))   # the first operation lost
                    inward = run[-1] + 1 if side == 0 else run[0] - 1          # the kept operation the cut run lies beyond
                    kept_of_run = int((~np.isin(run, lost)).sum())
                    if lo_of[rd] <= inward < hi_of[rd] and kept_of_run <= 2:
                        s.cut.append((int(rd), side, int(s.op[inward]), -1, "beyond", str(kept_of_run)))
                b = split[rd]
                run = lo_of[rd] + np.flatnonzero(s.opi[lo_of[rd]:hi_of[rd]] == s.opi[b])
                s.cut.append((int(rd), side, -1, int(s.op[b]), "bound", "first" if b == run[0] else "last" if b == run[-1] else "middle"))
            s.r, s.opi, s.op, s.p, s.base, s.qual = s.r[keep], s.opi[keep], s.op[keep], s.p[keep], s.base[keep], s.qual[keep]
            n = s.r.shape[0]
            starts = np.flatnonzero(np.concatenate([[True], s.r[1:] != s.r[:-1]])) if n else np.zeros(0, np.int64)
            stops = np.concatenate([starts[1:], [n]]) - 1 if n else starts
            for rd, edge in zip(s.r[starts], starts if side == 0 else stops):
                if applies[rd] and s.op[edge] == I:
                    run = (s.r == rd) & (s.opi == s.opi[edge])
                    s.op[run] = S
                    s.cut.append((int(rd), side, I, -1, "I_becomes_S", ""))
            onref = s.p >= 0
            big = np.iinfo(np.int64).max
            first = np.full(s.reads.shape[0], big, np.int64)
            np.minimum.at(first, s.r[onref], s.p[onref])
            last = np.full(s.reads.shape[0], -1, np.int64)
            np.maximum.at(last, s.r[onref], s.p[onref])
            s.pos = np.where(applies & (first < big), first, s.pos) if side == 0 else s.pos
            s.end = np.where(applies & (last >= 0), last + 1, s.end) if side == 1 else s.end

    def clipped_read(self, s: Sub, rd: int):
        """(pos, CIGAR, bases, qualities) of read ``rd`` of ``s``: the run lengths of its lines."""
        mine = np.flatnonzero(s.r == rd)
        cigar = []
        for k in mine:
            if cigar and cigar[-1][2] == s.opi[k]:
                cigar[-1][1] += 1
            else:
                cigar.append([int(s.op[k]), 1, s.opi[k]])
        q = mine[_QUERY[s.op[mine]]]
        return int(s.pos[rd]), [(o, n) for o, n, _ in cigar], bytes(s.base[q]).decode(), s.qual[q].tolist()

    # ---- the counting layer ----------------------------------------------------------------------
    def count(self, subs: Sequence[Sub]):
        """-> per technology table {position: [total, {(ref, alt): count}, left partials, right partials]}."""
        r, ref, text = self.rules, self.ref, self.reference
        tables: Tuple[dict, dict] = ({}, {})
        self.planted = planted = []

        def at(t, p):
            return tables[t].setdefault(int(p), [0, Counter(), Counter(), Counter()])
        for s in subs:
            counted = s.mapq[s.r] >= MAPQ_THRESHOLD if r.mapq_by_caller else np.ones(s.r.shape[0], bool)
            t, n = s.tech, s.r.shape[0]
            if n == 0:
                continue
            aligned = np.isin(s.op, (M, EQ, X) if r.eqx_counted else (M,)) & counted
            covered = aligned | ((s.op == N) & counted & (not r.n_uncounted))
            for p, c in zip(*np.unique(s.p[covered], return_counts=True)):
                at(t, p)[0] += int(c)
            refb = ref[np.where(aligned, s.p, 0)]
            snv = aligned & (s.base != refb) & (s.qual >= Q_THRESHOLD) & (s.base != ord("N")) & (refb != ord("N"))
            code = s.p[snv] * 65536 + refb[snv].astype(np.int64) * 256 + s.base[snv]
            for c, k in zip(*np.unique(code, return_counts=True)):
                at(t, c >> 16)[1][(chr((c >> 8) & 255), chr(c & 255))] += int(k)
            # per line: what lies before it in its read
            new = np.concatenate([[True], s.r[1:] != s.r[:-1]])
            start = np.maximum.accumulate(np.where(new, np.arange(n), 0))
            isq, onref = _QUERY[s.op], s.p >= 0
            q_before = np.cumsum(isq) - isq
            q_before -= q_before[start]
            ref_before = np.cumsum(onref) - onref
            ref_before -= ref_before[start]
            prev_q = rf._previous(isq, s.r)
            prev_a = rf._previous(np.isin(s.op, (M, EQ, X)), s.r)
            is_op = np.ones(n, bool) if r.ph_keep_index else ~np.isin(s.op, (H, P))
            opstart = np.concatenate([[True], (s.r[1:] != s.r[:-1]) | (s.opi[1:] != s.opi[:-1])])
            ci = np.cumsum(opstart & is_op) - (opstart & is_op)
            ci -= ci[start]
            n_ops = np.bincount(s.r[opstart & is_op], minlength=s.reads.shape[0])
            event = np.isin(s.op, (I, D)) & counted
            inc = 2 if (t == 0 and r.increment_2) else 1
            self.census.update("op_" + "MIDNSHP=X"[o] for o in s.op[opstart & counted])
            for a in np.flatnonzero(event & opstart):
                b = a
                while b < n and s.r[b] == s.r[a] and s.opi[b] == s.opi[a]:
                    b += 1
                length = b - a
                plant = int(s.pos[s.r[a]] - 1 + ref_before[a])
                c = at(t, plant)
                planted.append(plant)
                behind = int(s.op[a - 1]) if a > 0 and s.r[a - 1] == s.r[a] else -1
                if s.op[a] == D:
                    ref_allele = text[plant:plant + length + 1]
                    before = prev_q[a] if r.softclip_anchor else prev_a[a]
                    alt = chr(s.base[before]) if before >= 0 else text[plant]
                    if "N" in ref_allele or "N" in alt:
                        self.census["refused_N_in_ref" if "N" in ref_allele else "refused_N_in_alt"] += 1
                    elif before >= 0 and s.qual[before] < Q_THRESHOLD:
                        self.census["refused_quality"] += 1
                    else:
                        c[1][(ref_allele, alt)] += inc
                    self.census["D_with_rd_0"] += before < 0
                    self.census["D_behind_a_leading_S"] += bool(before >= 0 and s.op[before] == S)
                    continue
                inserted = bytes(s.base[a:b]).decode()
                ref_allele = text[plant]
                first, last, has_base = ci[a] == 0, ci[a] == n_ops[s.r[a]] - 1, q_before[a] > 0
                if first:
                    alt, quals, which = inserted, s.qual[a:b], 2
                    c[0] += int(r.lead_total)
                elif has_base:
                    alt, quals, which = chr(s.base[prev_q[a]]) + inserted, np.concatenate([[s.qual[prev_q[a]]], s.qual[a:b]]), 3 if last else 1
                else:
                    alt, quals, which = ref_allele + inserted, s.qual[a:b], 1
                self.census["I_as_operation_0"] += bool(first)
                self.census["I_as_the_last_operation"] += bool(last)
                self.census["I_behind_a_leading_H"] += bool(not first and not has_base)
                self.census["I_behind_a_leading_S"] += bool(behind == S)
                self.census["I_behind_P"] += behind == P
                self.census["I_behind_D"] += behind == D
                if "N" in ref_allele or "N" in alt:
                    self.census["refused_N_in_ref" if "N" in ref_allele else "refused_N_in_alt"] += 1
                elif quals.min() < Q_THRESHOLD:
                    self.census["refused_quality"] += 1
                else:
                    c[which][(ref_allele, alt)] += inc
        return self._resolved(tables)

    def _resolved(self, tables):
        for table in tables:                                             # the partials: exactly one key takes the count
            for p, c in table.items():
                adds: Counter = Counter()
                for which, fits in ((2, str.endswith), (3, str.startswith)):
                    for (_, palt), k in c[which].items():
                        hits = [key for key in c[1] if len(key[1]) >= len(palt) and fits(key[1], palt)]
                        self.census["%s_partial_with_%s" % ("left" if which == 2 else "right", ("0", "1", "2_or_more")[min(len(hits), 2)] + "_keys")] += 1
                        if len(hits) == 1:
                            adds[hits[0]] += k
                for key, k in adds.items():
                    c[1][key] += k
        return tables

    def flagged(self, tables) -> Set[int]:
        r, f32 = self.rules, np.float32
        out: Set[int] = set()
        if self.hybrid:
            for p, c in tables[0].items():
                other = tables[1].get(p)
                total = f32(c[0]) + f32(other[0] if other else 0)
                if total == 0:
                    continue
                for (ref, alt), k in c[1].items():
                    vi, vp = f32(k), f32(other[1].get((ref, alt), 0) if other else 0)
                    if (vi + vp) / total < f32(0.12):
                        continue
                    if len(ref) == 1 and len(alt) == 1:
                        out |= {p} if vi + vp >= 2 else set()
                    elif vi / f32(2) + vp >= 2:
                        out |= set(range(p, p + len(ref) + (0 if r.hybrid_exclusive else 1)))
                        self.census["key_of_%d" % max(len(ref), len(alt))] += 1
            return out
        for t, table in enumerate(tables):
            need = 4 if t == 0 else 2
            for p, c in table.items():
                if c[0] == 0:
                    continue
                for (ref, alt), k in c[1].items():
                    if f32(k) / f32(c[0]) < f32(0.12):
                        continue
                    if len(ref) == 1 and len(alt) == 1:
                        out |= {p} if k >= 2 else set()
                    elif k >= need:
                        self.census["key_of_%d" % max(len(ref), len(alt))] += 1
                        if max(len(ref), len(alt)) <= 100 or not r.limit_100:
                            out |= set(range(p, p + len(ref) + (1 if r.single_inclusive else 0)))
        return out

    def caps(self, lo: int, hi: int, hotspot: bool) -> List[float]:
        if hotspot:
            return [1000.0 if t == 1 else 10000.0 for t in self.tech]
        rate = lambda t: (100, 100) if t == 1 else (1000, 30)                                                  # noqa: E731
        return [rate(t)[0] / rate(t)[1] * (hi - lo) if hi - lo > rate(t)[1] else float(rate(t)[0]) for t in self.tech]

    def searcher(self, start: int, stop: int, lo: int, hi: int, hotspot: bool = False):
        """-> (status, flagged positions, the Subs, capped): selection, the clip, the window rule, counting and flagging of one
        searcher whose reads are fetched over [lo, hi)."""
        picked = [self.select(k, lo, hi, cap) for k, cap in enumerate(self.caps(lo, hi, hotspot))]
        if not any(p[0].size for p in picked):
            return "no_reads", set(), [], False
        subs = [self.sub(k, reads, capped, lo, hi) if not hotspot else self.sub_unclipped(k, reads, capped) for k, (reads, capped) in enumerate(picked)]
        first = min([int(s.pos.min()) for s in subs if s.reads.size] + [start]) - 10
        last = max(int(s.end.max()) for s in subs if s.reads.size)
        capped = any(c for _, c in picked)
        if first < 0 or last > len(self.reference):
            return "out_of_bounds", set(), subs, capped
        found = self.flagged(self.count(subs))
        if not hotspot:
            self.tile_census(start, stop, subs, found)
        return "ok", found, subs, capped

    def tile_census(self, start: int, stop: int, subs, found: Set[int]) -> None:
        """candidates.hip's tiles of one searcher: from the later of one before the first counted read and ``start - kReach`` to
        the earlier of the last counted end and ``stop + 1``; flagged positions are kept on [start - 1, stop + 1)."""
        counted = [(s.pos[s.mapq >= MAPQ_THRESHOLD], s.end[s.mapq >= MAPQ_THRESHOLD]) for s in subs]
        if not any(pos.size for pos, _ in counted):
            return
        lo = max(min(int(pos.min()) for pos, _ in counted if pos.size) - 1, start - 102)
        hi = min(max(int(end.max()) for _, end in counted if end.size), stop + 1)
        if lo >= hi:
            return
        tiles = -(-(hi - lo) // K_TILE)
        where = np.array(self.planted, np.int64) - lo
        inside = (where >= 0) & (where < tiles * K_TILE)
        self.census["candidate_tiles"] += tiles
        self.census["candidate_event_on_the_last_column_of_a_tile"] += int((inside & (where % K_TILE == K_TILE - 1)).sum())
        self.census["candidate_event_on_the_first_column_of_a_tile"] += int((inside & (where % K_TILE == 0)).sum())
        self.census["candidate_flagged_run_across_a_tile_edge"] += sum(lo + K_TILE * k in found and lo + K_TILE * k - 1 in found for k in range(1, tiles))
        self.census["candidate_flagged_run_across_flag_lo"] += int(start - 2 in found and start - 1 in found)

    def sub_unclipped(self, k, reads, capped):
        tech, self.tech[k] = self.tech[k], 0
        try:
            s = self.sub(k, reads, capped, 0, 0)
        finally:
            self.tech[k] = tech
        s.tech = tech
        return s

    def hotspots(self, start: int, stop: int) -> List[int]:
        size = 10000 if (self.two or self.tech[0] == 1) else 400
        out: Set[int] = set()
        self.tiles = []
        for b in range(start, stop, size):
            e = min(b + size, stop)
            status, found, subs, _ = self.searcher(b, e, b, e, hotspot=True)
            out |= {p for p in found if b <= p < e}
            counted = [(s.pos[s.mapq >= MAPQ_THRESHOLD], s.end[s.mapq >= MAPQ_THRESHOLD]) for s in subs]
            if status == "ok" and any(pos.size for pos, _ in counted):    # hotspots.hip: tiles from one before the first counted start
                lo = min(int(pos.min()) for pos, _ in counted if pos.size) - 1
                hi = max(int(end.max()) for _, end in counted if end.size)
                where = np.array(self.planted, np.int64) - lo
                self.tiles.append(np.bincount(where // K_TILE, minlength=-(-(hi - lo) // K_TILE)))
                self.census["event_on_the_last_column_of_a_tile"] += int((where % K_TILE == K_TILE - 1).sum())
                self.census["event_on_the_first_column_of_a_tile"] += int((where % K_TILE == 0).sum())
                self.census["flagged_run_across_a_chunk_edge"] += int(b > start and b in found and b - 1 in found)
                self.census["flagged_run_across_a_tile_edge"] += sum(lo + K_TILE * k in found and lo + K_TILE * k - 1 in found
                                                                     for k in range(1, self.tiles[-1].size))
        return sorted(out)

    # ---- the site layer --------------------------------------------------------------------------
    def runs(self, found: Set[int], start: int, stop: int) -> List[Tuple[int, int]]:
        p = np.array(sorted(found), np.int64)
        if p.size == 0:
            return []
        cut = np.flatnonzero(np.diff(p) != 1)
        a, b = p[np.concatenate([[0], cut + 1])], p[np.concatenate([cut, [p.size - 1]])] + 1
        if self.rules.strict_drop:
            ok = (a >= start) & (b <= stop)
            return [(int(x), int(y)) for x, y in zip(a[ok], b[ok])]
        a, b = np.maximum(a, start), np.minimum(b, stop)
        return [(int(x), int(y)) for x, y in zip(a, b) if x < y]

    def clusters(self, locations):
        limit = 80 if self.rules.limit_80 else 1 << 30
        out, cluster = [], []
        for a, b in locations:
            if b - a > limit and cluster:
                self.census["location_above_80_with_an_open_cluster"] += 1
                out.append(cluster)
                cluster = []
                continue
            self.census["location_above_80_with_an_empty_cluster"] += b - a > limit
            if cluster and not (a - cluster[-1][1] < 30 and len(cluster) < 1024):
                out.append(cluster)
                cluster = []
            cluster.append((a, b))
        return out + ([cluster] if cluster else [])

    def records(self, s: Sub, regions):
        """Per read of ``s``: (Success records [(allele, start, stop, min_q)], the last left partial, the last right partial)."""
        r, out = self.rules, []
        n = s.r.shape[0]
        new = np.concatenate([[True], s.r[1:] != s.r[:-1]]) if n else np.zeros(0, bool)
        start = np.maximum.accumulate(np.where(new, np.arange(n), 0)) if n else new
        onref = s.p >= 0
        ref_before = np.cumsum(onref) - onref
        ref_before = ref_before - ref_before[start] if n else ref_before
        holds = np.isin(s.op, (M, EQ, X, D))
        slot = np.where(holds, s.p, np.where(s.op == I, s.pos[s.r] - 1 + ref_before, -1)) if n else s.p
        is_op = np.ones(n, bool) if r.ph_keep_index else ~np.isin(s.op, (H, P))
        opstart = np.concatenate([[True], (s.r[1:] != s.r[:-1]) | (s.opi[1:] != s.opi[:-1])]) if n else new
        lo_of, hi_of = np.searchsorted(s.r, np.arange(s.reads.shape[0]), "left"), np.searchsorted(s.r, np.arange(s.reads.shape[0]), "right")
        for rd in range(s.reads.shape[0]):
            span = slice(lo_of[rd], hi_of[rd])
            mine = lo_of[rd] + np.flatnonzero(slot[span] >= 0)
            sl = slot[mine]
            held = set(s.p[mine[holds[mine]]].tolist())
            body = lo_of[rd] + np.flatnonzero(opstart[span] & is_op[span])
            ins = mine[(s.op[mine] == I) & opstart[mine]]
            partial_start = any(int(slot[k]) not in held for k in ins)
            seen_before = lambda k: int(slot[k]) in held or any(int(slot[j]) == int(slot[k]) for j in ins if j < k)      # noqa: E731
            partial_stop = any(body.size and k == body[-1] and seen_before(k) for k in ins)
            has = held | set(slot[ins].tolist())
            last = max(held) if held else -1
            qual = np.where(s.op[mine] == D, 60 if r.del_q60 else 0, s.qual[mine])
            text = np.where(s.op[mine] == D, 0, s.base[mine]).astype(np.uint8)
            only_d = {int(p) for p in set(sl.tolist()) if not (text[sl == p] != 0).any()}
            alleles, left, right = [], None, None
            for a, b in regions:
                if not (a <= last and s.pos[rd] < b) or last == -1:
                    self.census["status_Fail_outside"] += 1
                    continue
                if a not in has:
                    status, why = "L", "no_entry_at_start"
                elif a - 1 not in has:
                    status, why = ("L", "partial_start") if partial_start else ("S", "starts_at_start")
                elif b - 1 not in has:
                    status, why = "R", "no_entry_at_last"
                elif b not in has:
                    status, why = ("R", "partial_stop") if partial_stop else ("S", "ends_at_last")
                else:
                    status, why = "S", "spans"
                if a in only_d or b - 1 in only_d:
                    status, why = "F", "empty_entry_at_" + ("start" if a in only_d else "last")
                self.census["status_%s_%s" % (dict(S="Success", L="LeftPartial", R="RightPartial", F="Fail")[status], why)] += 1
                inside = (sl >= a) & (sl < b)
                chars = text[inside]
                record = (bytes(chars[chars != 0]).decode(), a, b, int(qual[inside].min()) if inside.any() else 10000)
                if status == "S":
                    alleles.append(record)
                    if len(record[0]) in (80, 81):
                        self.census["success_allele_of_%d" % len(record[0])] += 1
                elif status == "L":
                    left = record
                elif status == "R":
                    right = record
            out.append((alleles, left, right))
        return out

    def supports(self, subs: Sequence[Sub], regions):
        """-> ({region: candidate strings}, {region: {string: set of (BAM, read)}})."""
        r = self.rules
        candidates: Dict[tuple, set] = {}
        support: Dict[tuple, Dict[str, set]] = {}
        partials = []
        for k, s in enumerate(subs):
            for rd, (alleles, left, right) in enumerate(self.records(s, regions)):
                who = (k, rd)
                for allele, a, b, min_q in alleles:
                    if min_q >= Q_THRESHOLD and s.mapq[rd] >= MAPQ_THRESHOLD:
                        if "N" not in allele or not r.n_dropped_from_candidates:
                            candidates.setdefault((a, b), set()).add(allele)
                        self.census["N_allele_supported"] += "N" in allele
                        support.setdefault((a, b), {}).setdefault(allele, set()).add(who)
                if left is not None or right is not None:
                    partials.append((who, left if left is not None else right, left is not None))
        for who, (allele, a, b, _), is_left in partials:
            at = support.get((a, b), {})
            hits = [full for full in at if len(full) >= len(allele) and (full.endswith(allele) if is_left else full.startswith(allele))]
            self.census["supports_partial_joins_%s" % ("none", "one", "could_join_two")[min(len(hits), 2)]] += 1
            if len(hits) == 1:
                at[hits[0]].add(who)
        return candidates, support

    def gate(self, lo: int, hi: int) -> bool:
        """The project's coverage rule over a cluster's fetch [lo, hi) (DESIGN.md "Two BAMs"): the reads of BAM 0 that overlap it,
        mapped, primary, not QC-fail, not duplicate, a proper pair if paired; a column is every position one of their lines has;
        a line counts with mapq >= 10 and quality >= 13, a ``D`` / ``N`` line by the quality of the previous query line."""
        L = self.lines[0]
        f = L.flag
        ok = ((f & (0x4 | 0x100 | 0x800 | 0x200 | 0x400)) == 0) & (((f & 1) == 0) | ((f & 2) != 0)) & (L.pos < hi) & (L.end > lo)
        mine = ok[L.read] & (L.p >= 0)
        good = mine & (L.mapq[L.read] >= hy.MIN_COVERAGE_MAPQ)
        before = rf._previous(L.q >= 0, L.read)
        total = int((good & np.isin(L.op, (M, EQ, X)) & (L.qual >= hy.MIN_COVERAGE_BASEQ)).sum())
        total += int((good & np.isin(L.op, (D, N)) & (before >= 0) & (L.qual[np.maximum(before, 0)] >= hy.MIN_COVERAGE_BASEQ)).sum())
        return total > hy.MIN_COVERAGE * np.unique(L.p[mine]).shape[0]

    def find_sites(self, positions: Sequence[int]):
        """-> (regions of pass 1, regions of pass 2, sites [(start, stop, window start, [(allele, [(BAM, read in the BAM)])])],
        statistics, the clipped PacBio reads of every site's cluster {(BAM, read): (pos, CIGAR, bases, qualities)})."""
        st: Counter = Counter()
        limit = 80 if self.rules.limit_80 else 1 << 30
        p = np.asarray(positions, np.int64)
        locations: List[Tuple[int, int]] = []
        if p.size:
            gap = np.flatnonzero(~((np.diff(p) >= 0) & (np.diff(p) <= 30)))
            for a, b in zip(p[np.concatenate([[0], gap + 1])] - 15, p[np.concatenate([gap, [p.size - 1]])] + 15):
                st["active_regions"] += 1
                status, found, _, capped = self.searcher(int(a), int(b), max(0, int(a) - 75), int(b) + 75)
                st["regions_without_reads"] += status == "no_reads"
                st["regions_out_of_bounds"] += status == "out_of_bounds"
                st["regions_at_read_cap"] += status == "ok" and capped
                locations += self.runs(found, int(a), int(b))
        locations.sort()
        st["differing_regions_pass1"] = len(locations)
        pass2, sites, clipped = [], [], {}
        self.reassembled: Set[Tuple[int, int]] = set()       # two BAMs: the regions of the clusters that are reassembled
        self.gate_stats = Counter()
        for cluster in self.clusters(locations):
            st["clusters"] += 1
            a, b = cluster[0][0] - 15, cluster[-1][1] + 15 - 1
            status, found, subs, capped = self.searcher(a, b, a, b)
            st["clusters_without_reads"] += status == "no_reads"
            st["clusters_out_of_bounds"] += status == "out_of_bounds"
            st["clusters_at_read_cap"] += status == "ok" and capped
            regions = self.runs(found, a, b)
            pass2 += regions
            for s in subs:
                self.census.update("clip_%s_%s_%s_%s" % ("left" if side == 0 else "right", how, "MIDNSHP=X"[op if how != "bound" else bop], edge)
                                   for _, side, op, bop, how, edge in s.cut)
            open_gate = self.two and status == "ok" and self.gate(a, b)
            self.gate_stats["clusters_gate_passed"] += open_gate
            if not regions:
                continue
            if open_gate and len(regions) < REASSEMBLY_SIZE:          # reconciled onto Illumina alleles: hybrid_reference's alone
                self.gate_stats["clusters_reassembled"] += 1
                self.reassembled |= set(regions)
                continue
            self.gate_stats["clusters_skipped_for_size"] += open_gate
            candidates, support = self.supports(subs, regions)
            for s0, s1 in regions:
                ref_allele = self.reference[s0:s1]
                names = [ref_allele] + sorted((x for x in candidates.get((s0, s1), ()) if x != ref_allele), key=lambda x: x.encode("latin-1"))
                kept = [(x, sorted((k, int(subs[k].reads[rd])) for k, rd in support.get((s0, s1), {}).get(x, ()))) for x in names]
                self.census["site_whose_reference_allele_has_no_read"] += not kept[0][1]
                kept = [(x, who) for x, who in kept if who and len(x) <= limit]
                if not kept:
                    continue
                mid = (s0 + s1) // 2 - FEATURE_LENGTH // 2
                ws, we = min(mid, s0 - 1), max(mid + FEATURE_LENGTH, s1)
                if ws < 0 or we > len(self.reference):
                    st["sites_out_of_bounds"] += 1
                    continue
                self.census["site_with_4_or_more_alleles"] += len(kept) >= 4
                sites.append((s0, s1, ws, kept))
                for k, s in enumerate(subs):
                    if s.tech == 1:
                        for _, who in kept:
                            for kk, read in who:
                                if kk == k and (k, read) not in clipped:
                                    clipped[(s0, s1, k, read)] = self.clipped_read(s, int(np.searchsorted(s.reads, read)))
        st["differing_regions_pass2"] = len(pass2)
        st["sites"], st["alleles"] = len(sites), sum(len(x[3]) for x in sites)
        st["reads_gathered"] = sum(len(who) for x in sites for _, who in x[3])
        return locations, pass2, sites, {k: int(st[k]) for k in cr.STAT_KEYS}, clipped


# ------------------------------------------------------------------------------------------------
# where the oracle and the restatements differ
# ------------------------------------------------------------------------------------------------
PLAN_KEYS = cr.STAT_KEYS[:10]          # active_regions ... differing_regions_pass2: what both passes' searchers decide


def oracle_of(seed: int, route: str, pad: bool = True, rules: Rules = Rules(), stage: str = "sites") -> Oracle:
    want = restated(seed, route, pad)
    return Oracle(want["reference"], want["rows" if stage == "hotspots" else "site_rows"], route == "pacbio", route == "hybrid", rules)


def disagreements(seed: int, route: str, pad: bool = True, rules: Rules = Rules(), census: Counter = None) -> List[str]:
    """The names of what the oracle under ``rules`` and the restatements give differently on one input: the hotspot positions;
    the regions of both passes and the ten statistics the searchers decide; and, for one BAM, every site with its window, its
    alleles in order, and each allele's reads as (start, CIGAR, bases) -- for PacBio the clipped ones.  With two BAMs the coverage
    gate's statistics too, and the sites of every cluster that is not reassembled (gate shut, or ten regions and more); the
    reconcilement of PacBio reads onto Illumina alleles in the reassembled clusters (DESIGN.md "Two BAMs") has no table form here."""
    want = restated(seed, route, pad)
    out = []
    o = oracle_of(seed, route, pad, rules, "hotspots")
    start, stop = span_of(want["reference"], pad)
    out += ["hotspots"] if o.hotspots(start, stop) != want["hotspots"] else []
    plan = want["plan"]                                                  # the planner's counts: tiles and events per chunk
    out += ["tiles"] if (sum(t.size for t in o.tiles), sum(int(t.sum()) for t in o.tiles)) != (plan["tiles"], plan["event_capacity"]) else []
    if census is not None:
        census.update({"hotspot_" + k: v for k, v in o.census.items()})
    o = oracle_of(seed, route, pad, rules)
    pass1, pass2, sites, st, clipped = o.find_sites(want["positions"])
    ws = want["stats"]
    out += ["regions_pass1"] if pass1 != list(ws["regions_pass1"]) else []
    out += ["regions_pass2"] if pass2 != list(ws["regions_pass2"]) else []
    out += [k for k in PLAN_KEYS if st[k] != ws[k]]
    if census is not None:
        census.update(o.census)
    two = len(profiles_of(route)) == 2
    rows = want["site_rows"]
    mine = []
    for s0, s1, ws_, kept in sites:
        mine.append((s0, s1, ws_, [(text, [clipped[(s0, s1, k, r)][:3] if o.tech[k] == 1 else (rows[k][r][2], rows[k][r][3], rows[k][r][4]) for k, r in who])
                                   for text, who in kept]))
    plain = lambda r: (r.pos, [tuple(c) for c in r.cigar], r.seq)                                              # noqa: E731
    if two:
        out += [k for k in ("clusters_gate_passed", "clusters_reassembled", "clusters_skipped_for_size") if o.gate_stats[k] != ws[k]]
        if census is not None:
            census["sites_compared_with_two_bams"] += len(mine)
            census["sites_left_to_hybrid_reference"] += sum((s.start, s.stop) in o.reassembled for s in want["sites"])
        theirs = [(s.start, s.stop, s.window_start, [(text, [plain(s.reads0[i]) for i in i0] + [plain(s.reads1[i]) for i in i1])
                                                     for text, i0, i1 in s.alleles]) for s in want["sites"] if (s.start, s.stop) not in o.reassembled]
    else:
        out += [k for k in cr.STAT_KEYS[10:] if st[k] != ws[k]]
        theirs = [(s.start, s.stop, s.window_start, [(text, [plain(s.reads[i]) for i in idx]) for text, idx in s.alleles]) for s in want["sites"]]
    out += ["sites"] if [x[:3] for x in mine] != [x[:3] for x in theirs] else []
    out += ["alleles"] if [[t for t, _ in x[3]] for x in mine] != [[t for t, _ in x[3]] for x in theirs] else []
    out += ["reads"] if mine != theirs else []
    return out


@functools.lru_cache(maxsize=None)
def survey(route: str, pad: bool = True):
    """-> ({seed: disagreements}, census) over every seed of one route: the oracle against the restatements, the oracle's
    events per tile against the planner's counts, and how often each situation of DESIGN.md section 7r occurs."""
    found, census = {}, Counter()
    for seed in SEEDS:
        names = disagreements(seed, route, pad, census=census)
        if names:
            found[seed] = names
        st = restated(seed, route, pad)["stats"]
        census.update({"stat_" + k: 1 for k in stat_keys(route) if st[k] > 0})
        census.update({"plan_" + k: 1 for k, v in restated(seed, route, pad)["plan"].items() if v > 0})
        if len(profiles_of(route)) == 2:
            ran = st["clusters"] - st["clusters_without_reads"] - st["clusters_out_of_bounds"]
            census["stat_gate_shut"] += ran > st["clusters_gate_passed"]
            census["stat_clusters_skipped_for_size"] += st["clusters_skipped_for_size"] > 0
    return found, census


# ------------------------------------------------------------------------------------------------
# the census lines, and the read set built by hand for what no corpus reaches
# ------------------------------------------------------------------------------------------------
CENSUS_AT_LEAST_5 = tuple("op_" + x for x in "MIDNSHP=X") + tuple("hotspot_op_" + x for x in "MIDNSHP=X") + tuple(
    h + k for h in ("", "hotspot_") for k in (
        "I_as_operation_0", "I_behind_a_leading_S", "I_behind_a_leading_H", "I_behind_P", "I_behind_D", "I_as_the_last_operation",
        "D_with_rd_0", "D_behind_a_leading_S", "refused_N_in_ref", "refused_N_in_alt", "refused_quality",
        "left_partial_with_0_keys", "left_partial_with_1_keys", "left_partial_with_2_or_more_keys",
        "right_partial_with_0_keys", "right_partial_with_1_keys", "right_partial_with_2_or_more_keys")) + (
    "hotspot_key_of_100", "hotspot_key_of_101", "key_of_100", "success_allele_of_80", "success_allele_of_81",
    "location_above_80_with_an_empty_cluster", "location_above_80_with_an_open_cluster",
    "status_Fail_outside", "status_LeftPartial_no_entry_at_start", "status_LeftPartial_partial_start", "status_Success_starts_at_start",
    "status_RightPartial_no_entry_at_last", "status_RightPartial_partial_stop", "status_Success_ends_at_last", "status_Success_spans",
    "status_Fail_empty_entry_at_start", "status_Fail_empty_entry_at_last",
    "supports_partial_joins_one", "supports_partial_joins_none", "supports_partial_joins_could_join_two",
    "site_with_4_or_more_alleles", "site_whose_reference_allele_has_no_read", "N_allele_supported",
    "hotspot_event_on_the_last_column_of_a_tile", "hotspot_event_on_the_first_column_of_a_tile")
CENSUS_CLIP = tuple("clip_%s_%s" % (side, k) for side, inner, outer in (("left", "last", "first"), ("right", "first", "last")) for k in (
    ["inside_%s_%s" % (op, e) for op in "M=XIS" for e in (inner, "middle")] + ["whole_%s_%s" % (op, outer) for op in "M=XIS"]
    + ["bound_%s_%s" % (op, e) for op in "M=XDN" for e in ("first", "middle", "last")] + ["I_becomes_S_I_"]))
CENSUS_CLIP += tuple("clip_%s_%s" % (side, k) for side in ("left", "right") for k in (      # the cut in front of and behind D, N, I P I
    ["lost_%s_" % op for op in "DNP"] + ["beyond_%s_%d" % (op, n) for op in "DNP" for n in (1, 2)]))
CENSUS_TILES = ("candidate_event_on_the_last_column_of_a_tile", "candidate_event_on_the_first_column_of_a_tile",
                "hotspot_flagged_run_across_a_tile_edge", "candidate_flagged_run_across_a_tile_edge", "candidate_flagged_run_across_flag_lo")
CENSUS_TWO_BAMS = ("stat_gate_shut", "stat_clusters_gate_passed", "stat_clusters_reassembled", "stat_pacbio_reads_eligible",
                   "stat_pacbio_reads_reassigned", "stat_illumina_sites", "stat_clusters_skipped_for_size", "sites_compared_with_two_bams",
                   "sites_left_to_hybrid_reference")
CENSUS_ILLUMINA = ("hotspot_flagged_run_across_a_chunk_edge",)       # the other routes' 10 000-base chunk is the only one
CENSUS_ONCE = {            # what lives in the one corpus of the caps (PILE_SEED), per route: at least once
    "illumina": ("stat_clusters_at_read_cap",),
    "pacbio": ("stat_clusters_at_read_cap", "stat_regions_at_read_cap", "plan_chunks_at_read_cap"),
    "two_bams": ("stat_clusters_at_read_cap", "stat_regions_at_read_cap", "plan_chunks_at_read_cap"),
}
# reached by no corpus and by no hand-built set: a cluster's fetch [first - 15, last + 14) always holds the position of the event
# that flagged its first location, and the read that carries that event overlaps it
CENSUS_UNREACHABLE = ("stat_clusters_without_reads",)
# reached fewer than 5 times by the corpora of the route, and by the hand-built read sets below
CENSUS_BY_HAND = tuple((route, line) for route in ("illumina", "pacbio", "two_bams") for line in (
    "stat_sites_out_of_bounds", "stat_clusters_out_of_bounds")) + (
    ("pacbio", "status_RightPartial_partial_stop"), ("illumina", "stat_regions_without_reads"), ("two_bams", "stat_regions_without_reads"),
    ("illumina", "stat_regions_out_of_bounds"), ("pacbio", "candidate_flagged_run_across_a_tile_edge"),
    ("pacbio", "candidate_flagged_run_across_flag_lo"))
# reached by nothing here: pass 1 of one Illumina BAM fetches 180 bases and keeps 6 000 reads, a hotspot chunk 10 000; the existing
# hand cases of tests/test_candidates.py and tests/test_gpu_hotspots.py hold those caps
CENSUS_NOT_BUILT = (("illumina", "stat_regions_at_read_cap"), ("illumina", "plan_chunks_at_read_cap"))
HAND_SPAN = (239, 1039)        # the hotspot stage's span over the hand-built sets: its Illumina chunks meet at 639


@functools.lru_cache(maxsize=None)
def hand_built():
    """-> {name: (reference of 1 200 random bases, rows, positions)}: the read sets of the census lines the corpora do not reach.
    *ends*: at 20 an SNV under reads that begin at 3, less than 10 from the chromosome's start (``regions_out_of_bounds``); at
    1 150 an SNV whose feature window ends behind the chromosome (``sites_out_of_bounds``); at 300 an SNV under eight reads, three
    of which carry it, and two reads that end on it with a trailing ``I``: their last entry is the site's last position, nothing
    lies behind it and the insertion makes them partial (``RightPartial`` through ``partial_stop``); a position at 900 that no read
    is near (``regions_without_reads``).
    *cluster*: eight reads from 10 on, three with an SNV at 20, and the position 30: pass 1's region starts at 15 and its window
    at 5, the location (20, 21) makes a cluster that starts at 5, whose window starts before the chromosome
    (``clusters_out_of_bounds``).
    *edges*: 24 reads over [384, 720) under the positions 500, 530 ... 680, one active region [485, 695]: its tiles begin at
    485 - kReach = 383 and meet at 639, its flagged positions are kept from ``flag_lo`` = 484.  Six reads delete 639 - 643 (planted
    at 638, the first tile's last column; the flagged run 638 - 644 crosses the tile edge), six insert three bases behind 639 (the
    second tile's first column), six delete 484 - 487 (planted at 483: the run 483 - 488 crosses ``flag_lo - 1`` and leaves the
    region, so the strict rule drops it).  The hotspot stage over HAND_SPAN has the same tiles, and its Illumina chunks meet at
    639 too."""
    rng = np.random.default_rng(20261023)
    reference = "".join(rng.choice(list("ACGT"), size=1200))
    other = lambda p: "ACGT"[("ACGT".index(reference[p]) + 1) % 4]                                             # noqa: E731

    def snv_rows(rows, at, lo, hi):
        for k in range(8):
            text = reference[lo:hi]
            rows.append(_row(len(rows), lo, [(M, hi - lo)], text[:at - lo] + other(at) + text[at - lo + 1:] if k < 3 else text, REV * (k & 1)))
    ends: List[tuple] = []
    for at, lo, hi in ((20, 3, 43), (1150, 1110, 1190), (300, 270, 330)):
        snv_rows(ends, at, lo, hi)
    for k in range(2):
        ends.append(_row(len(ends), 270, [(M, 31), (I, 2)], reference[270:300] + other(300) + "GA"))
    cluster: List[tuple] = []
    snv_rows(cluster, 20, 10, 50)
    edges: List[tuple] = []
    for k in range(6):
        flag = REV * (k & 1)
        edges.append(_row(len(edges), 384, [(M, 336)], reference[384:720], flag))
        edges.append(_row(len(edges), 384, [(M, 255), (D, 5), (M, 76)], reference[384:639] + reference[644:720], flag))
        edges.append(_row(len(edges), 384, [(M, 256), (I, 3), (M, 80)], reference[384:640] + "GAT" + reference[640:720], flag))
        edges.append(_row(len(edges), 384, [(M, 100), (D, 4), (M, 232)], reference[384:484] + reference[488:720], flag))
    by_position = lambda rows: sorted(rows, key=lambda r: r[2])                                               # noqa: E731
    return {"ends": (reference, by_position(ends), [20, 300, 900, 1150]), "cluster": (reference, by_position(cluster), [30]),
            "edges": (reference, by_position(edges), list(range(500, 681, 30)))}


@functools.lru_cache(maxsize=None)
def hand_restated(route: str, name: str) -> Dict[str, object]:
    """The restatements on one hand-built set as ``route`` takes it (two BAMs: the same rows as either BAM): the hotspot positions
    over HAND_SPAN, and the sites of the set's own positions with their statistics."""
    reference, rows, positions = hand_built()[name]
    sets = [rows] * len(profiles_of(route))
    reads = [reads_of(r) for r in sets]
    st: Dict[str, object] = {}
    if route == "illumina":
        sites = cr.find_candidates(reads[0], reference, positions, Q_THRESHOLD, MAPQ_THRESHOLD, FEATURE_LENGTH, st)
    elif route == "pacbio":
        sites = pr.find_candidates(reads[0], reference, positions, Q_THRESHOLD, MAPQ_THRESHOLD, FEATURE_LENGTH, st)
    else:
        sites = hy.find_candidates(reads[0], reads[1], reference, positions, route == "hybrid", REASSEMBLY_SIZE, Q_THRESHOLD, MAPQ_THRESHOLD,
                                   FEATURE_LENGTH, st)
    hotspots = hr.find_hotspots(reads, reference, *HAND_SPAN, pacbio=route == "pacbio", hybrid_hotspot=route == "hybrid")
    return dict(reference=reference, rows=sets, positions=positions, sites=sites, stats=st, hotspots=hotspots)


HAND_STATS = {      # what each hand-built set is for, in every route
    "ends": dict(regions_out_of_bounds=1, sites_out_of_bounds=1, regions_without_reads=1, clusters_out_of_bounds=0, sites=1),
    "cluster": dict(regions_out_of_bounds=0, differing_regions_pass1=1, clusters_out_of_bounds=1, differing_regions_pass2=0, sites=0),
    "edges": dict(active_regions=1, differing_regions_pass1=1, differing_regions_pass2=1, sites=1),
}
