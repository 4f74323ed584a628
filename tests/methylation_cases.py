"""Inputs of the methylation tests (tests/test_methylation.py on the CPU, tests/test_gpu_methylation.py on the GPU): tables worked
by hand, one case per rule of DESIGN.md section 7m, and the edge stress on one 6 kb chromosome.

A hand row is ``Row(flag, position, CIGAR, bases, mm, ml, hp, mapq)`` on a reference of 200 bases: ``A`` everywhere but ``CG`` at 10,
20, 30, 50 and 198 and a lone ``C`` at 40.  ``mm`` is the text of the MM tag (None: no tag), ``ml`` the bytes of ML (None: no tag).
The expected COUNTS are written sparsely -- {(site position, class, counter): value}, what is not named is 0 -- and were worked out
from the rules, not from the code."""
from __future__ import annotations

import dataclasses
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from hello_amd import methylation as me
from hello_amd.bam import Mods, Reads
from tests.bam_writer import Read
from tests.gvcf_cases import D, H, I, M, N, S, reads_of

MOD, UNMOD, SUM = me.MODIFIED, me.UNMODIFIED, me.ML_SUM
REV = 0x10


def _plant(reference: str, at: int, text: str) -> str:
    return reference[:at] + text + reference[at + len(text):]


REF = "A" * 200
for _at, _text in ((10, "CG"), (20, "CG"), (30, "CG"), (40, "C"), (50, "CG"), (198, "CG")):
    REF = _plant(REF, _at, _text)
SITES = [10, 20, 30, 50, 198]


@dataclass
class Row:
    flag: int
    pos: int
    cigar: List[Tuple[int, int]]
    bases: str
    mm: Optional[bytes] = None
    ml: Optional[List[int]] = None
    hp: int = 0
    mapq: int = 60
    ml_type: bytes = b"C"                     # the BAM type of the ML array; anything but C is "not of type B:C"

    @property
    def end(self) -> int:
        return self.pos + max(1, sum(k for op, k in self.cigar if op in (M, D, N, 7, 8)))

    def tags(self) -> bytes:
        """The auxiliary fields of the record: HP first, then MM and ML as an instrument writes them."""
        out = b"HPC" + bytes([self.hp]) if self.hp else b""
        if self.mm is not None:
            out += b"MMZ" + self.mm + b"\0"
        if self.ml is not None:
            width = {b"C": "B", b"S": "H", b"c": "b"}[self.ml_type]
            out += b"MLB" + self.ml_type + struct.pack("<I", len(self.ml)) + struct.pack("<%d%s" % (len(self.ml), width), *self.ml)
        return out

    def parsed(self):
        return me.parse_mm(self.mm, bytes(self.ml) if self.ml is not None and self.ml_type == b"C" else None)


def read_set(rows: List[Row]) -> Tuple[Reads, Mods]:
    """Rows -> the arrays ``hello_bam_fetch_mods`` would give, the modifications through the restated parser."""
    reads = reads_of([(r.pos, r.cigar, r.bases, [30] * len(r.bases), r.flag, r.mapq) for r in rows])
    reads = dataclasses.replace(reads, hp=np.array([r.hp for r in rows], np.uint8))
    parsed = [r.parsed() for r in rows]
    cat = lambda k, dtype: np.concatenate([p[k] for p in parsed] + [np.zeros(0, dtype)]).astype(dtype)      # noqa: E731
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parsed])]).astype(np.int64)
    return reads, Mods(deltas=cat(0, np.int32), probs=cat(1, np.uint8), offsets=offsets,
                       mode=np.array([p[2] for p in parsed], np.uint8), state=np.array([p[3] for p in parsed], np.uint8))


def overlapping(rows: List[Row], lo: int, hi: int) -> List[Row]:
    """The rows a fetch of [lo, hi) returns: those whose reference span overlaps it."""
    return [r for r in rows if r.end > lo and r.pos < hi]


def bam_records(rows: List[Row]) -> List[Read]:
    return [Read("r%d" % i, r.pos, r.cigar, r.bases, [30] * len(r.bases), r.flag, r.mapq, tags=r.tags()) for i, r in enumerate(rows)]


@dataclass
class Case:
    name: str
    rows: List[Row]
    counts_at: Dict[Tuple[int, int, int], int]       # (site position, class, counter) -> value
    counts: Dict[str, int]                           # of me.METRIC_STATS, what is not 0 (belonging and n_sites are filled in)
    reference: str = REF
    sites: List[int] = field(default_factory=lambda: list(SITES))

    def cut(self) -> int:
        """Where the two-span run cuts the chromosome: through the middle of the first read."""
        return self.rows[0].pos + 2 if self.rows else 100

    def expected(self) -> np.ndarray:
        out = np.zeros((len(self.sites), 3, 3), np.int64)
        for (p, cls, counter), v in self.counts_at.items():
            out[self.sites.index(p), cls, counter] = v
        return out

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(me.METRIC_STATS, 0), belonging=len(self.rows), n_sites=len(self.sites), **self.counts)


M4, M14 = [(M, 4)], [(M, 14)]
AT8 = REF[8:12]                                      # AACG: site 10
AT8_14 = REF[8:22]                                   # AACGAAAAAAAACG: sites 10 and 20


def one(mm, ml, **kw) -> Row:
    return Row(0, 8, M4, AT8, mm, ml, **kw)


def two(mm, ml, **kw) -> Row:
    return Row(0, 8, M14, AT8_14, mm, ml, **kw)


HAND_TABLE: List[Case] = [
    # forward: the C at 10 is candidate 0.  Reverse: the stored G at 11 is candidate 0 from the right and names the site at 10
    Case("forward and reverse reads on one site",
         [Row(0, 8, [(M, 6)], REF[8:14], b"C+m,0;", [200]), Row(REV, 8, [(M, 6)], REF[8:14], b"C+m,0;", [100])],
         {(10, 0, MOD): 1, (10, 0, UNMOD): 1, (10, 0, SUM): 300}, dict(counting=2, observations=2)),
    # 2S 1M 3D 8M 2I 11M at 8: the clip's C is candidate 0, the site at 10 lies under the deletion, the insertion's C is
    # candidate 1, the C at 20 candidate 2 and the C at 30 candidate 3
    Case("a site under a deletion, an insertion and a soft clip",
         [Row(0, 8, [(S, 2), (M, 1), (D, 3), (M, 8), (I, 2), (M, 11)], "CG" + "A" + "A" * 8 + "CG" + REF[20:31], b"C+m,0,0,0,0;",
              [250, 251, 130, 20])],
         {(20, 0, MOD): 1, (20, 0, SUM): 130, (30, 0, UNMOD): 1, (30, 0, SUM): 20}, dict(counting=1, observations=2)),
    # 14M at 38: the read's C at 40 (the reference's lone C) and at 45 (over an A) are listed; over the site at 50 it says T
    Case("a read C over a non-CpG position, and a mismatching base over a CpG",
         [Row(0, 38, M14, "AACAAAACAAAATG", b"C+m,0,0;", [255, 255])], {}, dict(counting=1)),
    Case("ML 127 against 128", [Row(0, 48, M4, REF[48:52], b"C+m,0;", [127]), Row(0, 48, M4, REF[48:52], b"C+m,0;", [128])],
         {(50, 0, MOD): 1, (50, 0, UNMOD): 1, (50, 0, SUM): 255}, dict(counting=2, observations=2)),
    # each lists the second C alone; the first is unmodified for '.' and for no mode, and says nothing for '?'
    Case("mode '.', mode '?' and absent mode", [two(b"C+m.,1;", [200]), two(b"C+m?,1;", [200]), two(b"C+m,1;", [200])],
         {(10, 0, UNMOD): 2, (20, 0, MOD): 3, (20, 0, SUM): 600}, dict(counting=3, observations=5)),
    Case("an empty group C+m; in both modes", [one(b"C+m;", []), one(b"C+m?;", [])],
         {(10, 0, UNMOD): 1}, dict(counting=2, observations=1)),
    # delta-major: m5 h5 m2 h2
    Case("C+mh and C+hm interleaving", [two(b"C+mh,0,0;", [200, 1, 10, 2]), two(b"C+hm,0,0;", [1, 200, 2, 10])],
         {(10, 0, MOD): 2, (10, 0, SUM): 400, (20, 0, UNMOD): 2, (20, 0, SUM): 20}, dict(counting=2, observations=4)),
    Case("a group C+h before C+m", [two(b"C+h,0;C+m,1;", [9, 222])],
         {(10, 0, UNMOD): 1, (20, 0, MOD): 1, (20, 0, SUM): 222}, dict(counting=1, observations=2)),
    Case("a G-m group and a numeric code skipped", [one(b"G-m,0;C+76792,0;C+m,0;", [5, 6, 140])],
         {(10, 0, MOD): 1, (10, 0, SUM): 140}, dict(counting=1, observations=1)),
    Case("HP 0, 1, 2 and 3",
         [one(b"C+m,0;", [200], hp=0), one(b"C+m,0;", [100], hp=1), one(b"C+m,0;", [210], hp=2), one(b"C+m,0;", [50], hp=3)],
         {(10, 0, MOD): 2, (10, 0, UNMOD): 2, (10, 0, SUM): 560, (10, 1, UNMOD): 1, (10, 1, SUM): 100, (10, 2, MOD): 1, (10, 2, SUM): 210},
         dict(counting=4, observations=4)),
    Case("a CpG at the chromosome's last two bases",
         [Row(0, 196, M4, REF[196:200], b"C+m,0;", [150]), Row(REV, 196, M4, REF[196:200], b"C+m,0;", [60])],
         {(198, 0, MOD): 1, (198, 0, UNMOD): 1, (198, 0, SUM): 210}, dict(counting=2, observations=2)),
    Case("a C at the very last base", [Row(0, 196, M4, "AAAC", b"C+m,0;", [255])], {}, dict(counting=1),
         reference=_plant(REF, 198, "AC"), sites=SITES[:4]),
    # no ';'; an unknown base; a delta that is no number; no code; two matching groups; no ML; ML of another type; ML of another
    # length; a delta of 2^31; and the second candidate of a read that has one (found on the device)
    Case("each bad-modification case",
         [one(b"C+m,0", [1]), one(b"X+m,0;", [1]), one(b"C+m,a;", [1]), one(b"C+,0;", [1]), one(b"C+m,0;C+mh,0;", [1, 2, 3]),
          one(b"C+m,0;", None), one(b"C+m,0;", [1], ml_type=b"S"), one(b"C+m,0;", [1, 2]), one(b"C+m,2147483648;", [1]),
          one(b"C+m,1;", [1])], {}, dict(reads_bad_mods=10)),
    Case("a hard-clipped read", [Row(0, 8, [(H, 3), (M, 4)], AT8, b"C+m,0;", [200])], {}, dict(reads_hard_clipped=1)),
    Case("an uncounted read", [one(b"C+m,0;", [200], mapq=5), Row(0x400, 8, M4, AT8, b"C+m,0;", [200]), Row(0x100, 8, M4, AT8, b"C+m,0;", [200])],
         {}, {}),
    Case("a read without MM, and MM without a C+m group", [one(None, None), one(b"C+h,0;", [3]), one(b"C-m,0;", [3])],
         {}, dict(reads_no_mods=3)),
]


# ---- the edge stress: one 6 kb chromosome ---------------------------------------------------------------------------------------
LENGTH = 6000
SPAN = 1000
LONG_AT, LONG = 300, 1500                          # the long reads: over CCCG repeated, across the span edge at 1 000
RUN_AT = 4000                                      # CG repeated 150 times: reads listing 63, 64, 65 and 130 bases
PILE_AT, PILE = 4500, 300                          # 300 copies of a 20-base read on the site at 4 509
SHARE = 1024                                       # kMethShare of methylation.hip: more listed bases go to a scratch slice


def mm_of(stored: str, reverse: bool, wanted: List[int], mode: str = "") -> bytes:
    """The MM text that lists the stored indices ``wanted`` of a read (each a candidate: C, or G of a reverse read)."""
    at = [i for i, b in enumerate(stored) if b == ("G" if reverse else "C")]
    if reverse:
        at = at[::-1]
    ordinals = sorted(at.index(i) for i in wanted)
    deltas = [o - (ordinals[k - 1] + 1 if k else 0) for k, o in enumerate(ordinals)]
    return b"C+m" + mode.encode() + b"".join(b",%d" % d for d in deltas) + b";"


def cpgs_of(stored: str, reverse: bool) -> List[int]:
    """The stored indices an instrument lists: the C of every CG of the read, or for a reverse read the G (the C of its own strand)."""
    return [i + reverse for i in range(len(stored) - 1) if stored[i:i + 2] == "CG"]


def stress(seed: int = 13):
    """-> (reference, rows sorted by position): what tests/test_gpu_methylation.py's edge stress asserts really occurs."""
    rng = np.random.default_rng(seed)
    reference = "".join(rng.choice(list("ACGT"), size=LENGTH))
    reference = _plant(reference, LONG_AT, "CCCG" * (LONG // 4))
    reference = _plant(reference, 2047, "CG")                             # the C is the last position of a 64-position word
    reference = _plant(reference, 2112, "CG")                             # and the first
    reference = _plant(reference, RUN_AT, "CG" * 150)
    reference = _plant(reference, 4400, "AT" * 10)
    reference = _plant(reference, PILE_AT, "A" * 9 + "CG" + "A" * 9)
    reference = _plant(reference, 0, "CG")
    reference = _plant(reference, LENGTH - 2, "CG")
    reference = _plant(reference, 5000, reference[5000:5100].lower())
    rows: List[Row] = []

    def add(flag, pos, cigar, inserted="CG", mode=None, hp=None, wanted=None):
        bases, p = [], pos
        for op, k in cigar:
            if op == M:
                bases.append(reference[p:p + k].upper())
                p += k
            elif op in (I, S):
                bases.append((inserted * k)[:k])
            elif op in (D, N):
                p += k
        stored, reverse = "".join(bases), bool(flag & REV)
        wanted = cpgs_of(stored, reverse) if wanted is None else wanted
        mode = ("", ".", "?")[int(rng.integers(0, 3))] if mode is None else mode
        rows.append(Row(flag, pos, cigar, stored, mm_of(stored, reverse, wanted, mode), [int(x) for x in rng.integers(0, 256, size=len(wanted))],
                        int(rng.integers(0, 4)) if hp is None else hp))
        return rows[-1]
    for n, pos in enumerate(range(0, LENGTH - 150, 37)):                  # background: 150-base reads, every second reverse
        add(REV if n % 2 else 0, pos, [(M, 150)])
    add(0, LENGTH - 20, [(M, 20)])                                         # the last site of the chromosome (the first: the read at 0)
    for edge in (SPAN, 2 * SPAN, 3 * SPAN, 2048):                          # clips, insertions and deletions across the edges
        add(0, edge - 70, [(S, 5), (M, 60), (D, 20), (M, 30), (I, 6), (M, 60)])
        add(REV, edge - 40, [(S, 4), (M, 30), (I, 2), (M, 30), (S, 3)])
    for flag in (0, 0, REV):                                               # every C (1 125: two scratch slices) or G (375) listed
        r = add(flag, LONG_AT, [(M, LONG)], wanted=[])
        every = [i for i, b in enumerate(r.bases) if b == ("G" if flag else "C")]
        rows.pop()
        add(flag, LONG_AT, [(M, LONG)], wanted=every, mode="")
    for n in (63, 64, 65, 130):
        add(0, RUN_AT, [(M, 2 * n)], mode="?")
        add(REV, RUN_AT + 2, [(M, 2 * n)], mode=".")
    add(0, 4400, [(M, 20)], wanted=[])                                     # a read with no C at all
    for n in range(PILE):
        add(REV if n % 3 == 0 else 0, PILE_AT, [(M, 20)], hp=n % 4)
    late = add(0, 4600, [(M, 40)])                                         # a delta pointing one past the last candidate
    late.mm = b"C+m,%d;" % late.bases.count("C")
    late.ml = [77]
    rows.sort(key=lambda r: r.pos)
    return reference, rows


# ---- the scan's carry: a chromosome of three rounds of the site scan ------------------------------------------------------------
CARRY_LENGTH = 2 * 65536 + 48                      # 2 049 words: two full rounds of 1 024 words and a third of one word
CARRY_SPAN = 50000
# A CpG takes two positions, so of the last bit of a round and the first bit of the next only one can be a site: the first edge has
# its site on the last bit (65 535) and the next at 65 537, the second on bit 62 (131 070) and on the first bit (131 072).
CARRY_NAMED = (0, 65535, 65537, 131070, 131072, CARRY_LENGTH - 2)


def carry(seed: int = 29):
    """-> (reference, sites, rows sorted by position): a text without G but for the CG planted at the named sites and at 40 seeded
    positions, a read of 20 to 150 bases over every site on alternating strands that lists its CpGs, and one read across each of
    the two round edges."""
    rng = np.random.default_rng(seed)
    reference = "".join(rng.choice(list("ACT"), size=CARRY_LENGTH))
    sites = set(CARRY_NAMED)
    for p in (int(p) for p in rng.integers(3, CARRY_LENGTH - 4, size=40)):
        if all(abs(p - s) > 2 for s in sites):
            sites.add(p)
    for p in sites:
        reference = _plant(reference, p, "CG")
    rows: List[Row] = []

    def add(flag, pos, n):
        stored, reverse = reference[pos:pos + n], bool(flag & REV)
        wanted = cpgs_of(stored, reverse)
        rows.append(Row(flag, pos, [(M, n)], stored, mm_of(stored, reverse, wanted, ("", ".", "?")[len(rows) % 3]),
                        [int(x) for x in rng.integers(0, 256, size=len(wanted))], len(rows) % 4))
    for k, p in enumerate(sorted(sites)):
        n = int(rng.integers(20, 151))
        add(REV if k % 2 else 0, max(0, min(p - int(rng.integers(0, n - 1)), CARRY_LENGTH - n)), n)      # over p and p + 1
    add(0, 65536 - 50, 100)
    add(REV, 131072 - 40, 70)
    rows.sort(key=lambda r: r.pos)
    return reference, np.array(sorted(sites), np.int64), rows
