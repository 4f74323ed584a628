"""Inputs of the tests of the split alignments (tests/test_sv_split.py on the CPU, tests/test_gpu_sv_split.py on the GPU): cases
worked by hand, one per rule of DESIGN.md section 7q, at min_size 5 and flank 3; a stress set on one chromosome of 2 600 positions;
and a seeded fuzz of tags built from random segment sets, one in four mutated byte-wise into garbage.

A row is a row of tests/sv_cases.py with the read's SA text behind it: (name_hash, flag, position, CIGAR, bases, qualities, mapq,
hp, tag).  The hand cases' expected rows were worked out from the rules, not from the code."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from hello_amd import sv
from hello_amd.bam import Splits
from tests import sv_cases as sc
from tests.sv_cases import D, H, I, M, REV, S  # noqa: F401

DEL, INS, DUP, INV3, INV5, BND = sv.DEL, sv.INS, sv.DUP, sv.INV3, sv.INV5, sv.BND
CONTIGS = ("chr1", "chr2", "chrUn_1")
OWN = 0
HAND = dict(sc.HAND)


def sa(rname: str, pos0: int, strand: str, cigar: str, mapq: int = 60, nm: int = 0) -> bytes:
    """One entry of an SA tag for a segment that starts at the 0-based ``pos0``."""
    return b"%s,%d,%s,%s,%d,%d;" % (rname.encode(), pos0 + 1, strand.encode(), cigar.encode(), mapq, nm)


def tagged(row: tuple, tag: bytes = b"") -> tuple:
    return tuple(row) + (bytes(tag),)


def split_set(rows) -> Tuple[object, Splits]:
    """Rows -> (the Reads, the Splits) ``fetch_with_sa`` would give."""
    text = b"".join(r[8] for r in rows)
    offsets = np.concatenate([[0], np.cumsum([len(r[8]) for r in rows])]).astype(np.int64)
    return sc.read_set([r[:8] for r in rows]), Splits(np.frombuffer(text, np.uint8).copy(), offsets)


def spans_of(rows, length: int, cuts=()):
    """[(reads, splits, lo, hi)]: the chromosome whole, or cut at ``cuts``, each span with the rows a fetch of it returns."""
    edges = [0] + list(cuts) + [length]
    return [split_set(sc.overlapping(rows, lo, hi)) + (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]


@dataclass
class Case:
    name: str
    reference: str
    rows: List[tuple]
    signatures: List[Tuple[int, ...]]                # every row of sv.SIGNATURE_COLUMNS, sorted
    clusters: List[Tuple[int, ...]]                  # (type, pos, len, DV, SR, DP, DR) of every candidate
    split_status: List[int]
    counts: Dict[str, int] = field(default_factory=dict)     # of sv.SPLIT_COUNT_NAMES, what is not 0

    def cut(self) -> int:
        return self.rows[0][2] + 2

    def want_counts(self) -> Dict[str, int]:
        return dict(dict.fromkeys(sv.SPLIT_COUNT_NAMES, 0), **self.counts)


# ---- the hand cases ----------------------------------------------------------------------------------------------------------------
TANDEM = sc.TANDEM                                   # TCAGT CCGTA CCGTA GTTCAGATCA: CCGTA at 5 and at 10
_DEL8 = [(M, 8), (D, 5), (M, 8)]


def _hand_reference() -> str:
    """300 random bases in which no deletion of the cases below can move: the base before each differs from its last one."""
    rng = np.random.default_rng(41)
    ref = list("".join(rng.choice(list("ACGT"), size=300)))
    for at, base in ((114, "A"), (129, "C"), (119, "G"), (144, "A"), (159, "C"), (69, "A"), (102, "C")):
        ref[at] = base
    return "".join(ref)


PLAIN = _hand_reference()
_P15 = [(M, 15), (S, 15)]                            # a primary of 30 bases whose first 15 align at 100: it leaves the reference at 115


def _one(name, rows, signatures, status, clusters=(), reference=PLAIN, **counts) -> Case:
    n = sum(1 for r in rows if r[8])
    base = dict(split_reads=n, junctions=0)
    base.update(counts)
    return Case(name, reference, rows, sorted(signatures), list(clusters), list(status), {k: v for k, v in base.items() if v})


HAND_TABLE: List[Case] = [
    # read 1 carries the deletion of the second copy as 5D: 7p moves it from 10 to 5.  Read 2 is split there: its primary ends at
    # 10, its other segment begins at 15, no base of the read lies between: d = net = 5, a DEL at 10 that moves over j < 10 - 2 by
    # five, as read 1's.  Spanning depth at 5: read 1 covers 5 .. 20, read 2's primary (2 .. 10) covers 5 .. 7: DP 2, DR 2 - (2 - 1)
    _one("a forward deletion at the right copy joins the 5D of the same event",
         [tagged(sc.row(1, TANDEM, 2, _DEL8)), tagged(sc.row(2, TANDEM, 2, [(M, 8), (S, 8)]), sa("chr1", 15, "+", "8S8M"))],
         [(DEL, 5, 5, 5, 0, 1, 0, 0), (DEL, 5, 5, 5, 1, -1, 0, 0)], [0, 2], [(DEL, 5, 5, 2, 1, 2, 1)], TANDEM,
         junctions=1, split_signatures=1),
    # on the reverse strand the read begins with the segment at 15: A = the entry (exit 15), B = the primary (entry 10)
    _one("the same event on reverse-strand reads",
         [tagged(sc.row(1, TANDEM, 2, _DEL8, REV)), tagged(sc.row(2, TANDEM, 2, [(M, 8), (S, 8)], REV), sa("chr1", 15, "-", "8S8M"))],
         [(DEL, 5, 5, 5, 0, 1, 1, 0), (DEL, 5, 5, 5, 1, -1, 1, 0)], [0, 2], [(DEL, 5, 5, 2, 1, 2, 1)], TANDEM,
         junctions=1, split_signatures=1),
    # the entry's aligned bases begin at 17, three before the primary's end at 20: B enters at 100 + 3, d = 103 - 70 = 33
    _one("an overlap is trimmed from the second segment",
         [tagged(sc.row(1, PLAIN, 50, [(M, 20), (S, 10)]), sa("chr1", 100, "+", "17S13M"))],
         [(DEL, 70, 33, 0, 0, -1, 0, 0)], [2], junctions=1, split_signatures=1),
    # five of B's five bases overlap: nothing is left of it
    _one("an overlap that leaves the second segment shorter than the flank",
         [tagged(sc.row(1, PLAIN, 50, [(M, 20), (S, 10)]), sa("chr1", 100, "+", "15S5M10S"))],
         [], [1], junctions=1, junctions_dropped=1),
    # the read goes on at 90, 25 before where it left: d = -25
    _one("a duplication", [tagged(sc.row(1, PLAIN, 100, _P15, hp=2), sa("chr1", 90, "+", "15S15M"))],
         [(DUP, 90, 25, 0, 0, -1, 0, 2)], [2], junctions=1, split_signatures=1),
    # A forward leaves at 115; B reverse 200 .. 215 is entered at its end, 215: right ends joined
    _one("an inversion junction that joins two right ends", [tagged(sc.row(1, PLAIN, 100, _P15), sa("chr1", 200, "-", "15M15S"))],
         [(INV3, 115, 100, 0, 0, -1, 0, 0)], [2], junctions=1, split_signatures=1),
    # the primary is reverse and first on the read (its clip leads on the reference): it leaves at its start, 100; B forward enters at 200
    _one("an inversion junction that joins two left ends",
         [tagged(sc.row(1, PLAIN, 100, [(S, 15), (M, 15)], REV), sa("chr1", 200, "+", "15S15M"))],
         [(INV5, 100, 100, 0, 0, -1, 1, 0)], [2], junctions=1, split_signatures=1),
    # ten bases of the read between the segments, none of the reference: net = 0 - 10
    _one("an insertion-like junction", [tagged(sc.row(1, PLAIN, 100, [(M, 15), (S, 25)]), sa("chr1", 115, "+", "25S15M"))],
         [(INS, 115, 10, 0, 0, -1, 0, 0)], [2], junctions=1, split_signatures=1),
    _one("a breakend to another chromosome", [tagged(sc.row(1, PLAIN, 100, _P15), sa("chr2", 500, "+", "15S15M"))],
         [(BND, 115, 1, 500, 0, -1, 0, 0)], [2], junctions=1, split_signatures=1),
    # the tag names the third segment first; on the read the order is primary (0 .. 15), 130 .. 145 (15 .. 30), 160 .. 175 (30 .. 45)
    _one("three segments with two junctions",
         [tagged(sc.row(1, PLAIN, 100, [(M, 15), (S, 30)]), sa("chr1", 160, "+", "30S15M") + sa("chr1", 130, "+", "15S15M15S"))],
         [(DEL, 115, 15, 0, 0, -1, 0, 0), (DEL, 145, 15, 0, 0, -2, 0, 0)], [2], junctions=2, split_signatures=2),
    _one("a hard-clipped supplementary entry", [tagged(sc.row(1, PLAIN, 100, _P15), sa("chr1", 130, "+", "15H15M"))],
         [(DEL, 115, 15, 0, 0, -1, 0, 0)], [2], junctions=1, split_signatures=1),
    _one("a partner one below the mapq threshold", [tagged(sc.row(1, PLAIN, 100, _P15), sa("chr1", 130, "+", "15S15M", 9))],
         [], [1], junctions=1, junctions_dropped=1),
    # two reads each: net 5 is a deletion with DV 2, SR 2; net 4 is nothing.  The second read is reverse: its primary 15M15S lies
    # second on the read (qs 15), the entry 15S15M first: A = the entry leaves at its start 120, B = the primary is entered at its
    # end 115, d = 120 - 115.  Depth at 115: all four primaries end there and cover 103 .. 112: DP 0, DR 0
    _one("net at min_size and one below",
         [tagged(sc.row(1, PLAIN, 100, _P15), sa("chr1", 120, "+", "15S15M")), tagged(sc.row(2, PLAIN, 100, _P15, REV), sa("chr1", 120, "-", "15S15M")),
          tagged(sc.row(3, PLAIN, 100, _P15), sa("chr1", 119, "+", "15S15M")), tagged(sc.row(4, PLAIN, 100, _P15), sa("chr1", 119, "+", "15S15M"))],
         [(DEL, 115, 5, 0, 0, -1, 0, 0), (DEL, 115, 5, 0, 1, -1, 1, 0)], [2, 2, 1, 1], [(DEL, 115, 5, 2, 2, 0, 0)],
         junctions=4, junctions_small=2, split_signatures=2),
]

HAND_VCF_LINES = (
    "chr1\t5\t.\tT\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-5;END=10;SUPPORT=2;CIPOS=0,0;CILEN=0,0;STRANDS=2,0;SR=1\t"
    "GT:GQ:DR:DV:PL:HPS\t%s:%d:1:2:%d,%d,%d:2,0,0\n")


# ---- the stress: one chromosome of 2 600 positions ------------------------------------------------------------------------------------
LENGTH = sc.LENGTH
STRESS = dict(sc.STRESS)                             # min_size 10, flank 5, cluster_gap 20, min_support 2
SHIFTS = sc.SHIFTS
SHIFT_AT = sc.SHIFT_AT
BAD_CAUSES = ("trailing bytes", "no semicolon", "empty rname", "pos 0", "eleven digits", "strand", "unknown operation", "count 0",
              "clip inside", "no aligned base", "no reference base", "mapq 256", "no NM", "bytes behind NM", "other length",
              "past the end", "primary past the end", "empty entry")


def _pad_to(entry: bytes, total: int, rname_at: int = 0) -> bytes:
    """``entry`` with its rname lengthened so that the text has ``total`` bytes."""
    more = total - len(entry)
    assert more >= 0
    return entry[:rname_at] + b"x" * more + entry[rname_at:]


def stress(seed: int = 29):
    """-> (reference, rows sorted by position, named): sv_cases.stress() with its reads untagged, and split reads beside them."""
    reference, rows, named = sc.stress(seed)
    rows = [tagged(r) for r in rows]
    named = dict(named)
    next_name = [max(r[0] for r in rows) + 1]

    def add(situation: str, pos: int, cigar, tag: bytes, flag: int = 0, mapq: int = 60, hp: int = 0):
        name = next_name[0]
        next_name[0] += 1
        rows.append(tagged(sc.row(name, reference, pos, cigar, flag, mapq, hp), tag))
        named.setdefault(situation, []).append(name)
        return name

    p40 = [(M, 40), (S, 20)]                          # 60 bases, the first 40 aligned
    far = sa("chr1", 2000, "+", "40S20M")             # a deletion of hundreds of bases: never small, never clustered with another
    # the shifts of 0, 63, 64 and 65 of sv_cases, as splits: the read leaves at the deletion's start and goes on 12 later; beside
    # the 12D reads of sv_cases each makes a cluster of two
    for k in SHIFTS:
        at = SHIFT_AT[k]
        add("split_shift%d" % k, at - k - 10, [(M, k + 10), (S, 20)], sa("chr1", at + 12, "+", "%dS20M" % (k + 10)), hp=1)
    # the left segment's start stops the move: 40 bases before the deletion in a stretch that would let it move by 65
    add("split_stopped", sc.STOPPED_AT - 40, p40, sa("chr1", sc.STOPPED_AT + 12, "+", "40S20M"))
    # lower case and N in the repeat
    add("split_n_in_repeat", sc.N_AT - 40, p40, sa("chr1", sc.N_AT + 12, "+", "40S20M"))
    # tags of 63, 64, 65 and 129 bytes (one entry; the rname is made longer, which makes it unknown: a BND with tid -1)
    entry = sa("q", 2000, "+", "40S20M")
    for total in (63, 64, 65, 129):
        add("bytes%d" % total, 1100 + total, p40, _pad_to(entry, total))
    # two entries, the first 58, 60, 64 and 65 bytes long with its ';': the second entry's number "2101" lies on bytes 63 .. 66, the
    # second entry begins at byte 60 and runs over byte 64, and the first ';' is the last byte of a 64-byte step and the first of the next
    second = sa("chr1", 2100, "+", "50S10M")
    for i, (first_len, what) in enumerate(((58, "number_straddles"), (60, "entry_straddles"), (64, "semicolon_at_63"), (65, "semicolon_at_64"))):
        add(what, 1250 + i, p40, _pad_to(sa("chr2", 700, "+", "40S10M10S"), first_len) + second)
    # 7 and 8 entries: 8 segments of 10 bases each, and one more
    seven = b"".join(sa("chr1", 2150 + 40 * i, "+", "%dS10M%s" % (10 * i, "%dS" % (70 - 10 * i) if i < 7 else "")) for i in range(1, 8))
    add("seven_entries", 2150, [(M, 10), (S, 70)], seven)
    eight = b"".join(sa("chr1", 2151 + 40 * i, "+", "%dS10M%s" % (10 * i, "%dS" % (80 - 10 * i) if i < 8 else "")) for i in range(1, 9))
    add("eight_entries", 2151, [(M, 10), (S, 80)], eight)
    # pos of 2^31 - 1 (on another chromosome: one base long) and of eleven digits
    add("pos_max", 1300, p40, b"chr2,2147483647,+,59S1M,60,0;")
    add("pos_eleven", 1301, p40, b"chr2,21474836470,+,40S20M,60,0;")
    # e == length and length + 1
    add("ends_at_length", 1400, p40, sa("chr1", LENGTH - 20, "+", "40S20M"))
    add("ends_past_length", 1401, p40, sa("chr1", LENGTH - 19, "+", "40S20M"))
    # a read over two spans (the cut at 1 400 runs through it)
    add("over_two_spans", 1380, p40, far)
    # an unknown rname
    add("unknown_rname", 1500, p40, sa("chrZ", 10, "+", "40S20M"))
    # a read that does not count carries a tag; a tag on a read with an event of its own
    add("not_counting", 1510, p40, far, mapq=5)
    add("both_kinds", 1520, [(M, 20), (D, 12), (M, 20), (S, 20)], far, hp=2)
    # every BAD_SA cause once
    good = sa("chr1", 2000, "+", "40S20M")
    causes = {
        "trailing bytes": good + b"x", "no semicolon": good[:-1], "empty rname": b",2001,+,40S20M,60,0;", "pos 0": b"chr1,0,+,40S20M,60,0;",
        "eleven digits": b"chr1,2001,+,40S20M,60,00000000001;", "strand": b"chr1,2001,*,40S20M,60,0;",
        "unknown operation": b"chr1,2001,+,40S20B,60,0;", "count 0": b"chr1,2001,+,40S0I20M,60,0;", "clip inside": b"chr1,2001,+,20S10M20S10M,60,0;",
        "no aligned base": b"chr1,2001,+,60S20D,60,0;", "no reference base": b"chr1,2001,+,40S20I,60,0;", "mapq 256": b"chr1,2001,+,40S20M,256,0;",
        "no NM": b"chr1,2001,+,40S20M,60;", "bytes behind NM": b"chr1,2001,+,40S20M,60,0,;", "other length": b"chr1,2001,+,40S21M,60,0;",
        "past the end": sa("chr1", LENGTH - 10, "+", "40S20M"), "empty entry": good + b";",
    }
    for i, cause in enumerate(BAD_CAUSES):
        if cause == "primary past the end":
            add("bad: " + cause, LENGTH - 30, p40, sa("chr1", 100, "+", "40S20M"))
        else:
            add("bad: " + cause, 1600 + i, p40, causes[cause])
    rows.sort(key=lambda r: r[2])
    return reference, rows, named


# ---- the fuzz ------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(32))
FUZZ_LENGTH = 1500
FUZZ = dict(min_size=4, flank=2, mapq_threshold=10, cluster_gap=20, len_ratio_percent=70, min_support=2)


def fuzz(seed: int):
    """-> (reference, rows): 24 reads of 60 bases cut into 2 to 5 segments at random places of three chromosomes, strands and
    mapqs; the tag lists the other segments in random order; one tag in four has 1 to 3 bytes replaced, inserted or removed."""
    rng = np.random.default_rng(1000 + seed)
    reference = "".join(rng.choice(list("ACGTacgtN"), size=FUZZ_LENGTH, p=[.22, .22, .22, .22, .02, .02, .02, .02, .04]))
    for at in range(100, FUZZ_LENGTH - 100, 150):          # short tandem repeats for the moves to the left
        unit = reference[at:at + 3]
        reference = reference[:at] + unit * 8 + reference[at + 24:]
    rows = []
    total = 60
    for name in range(1, 25):
        n_seg = int(rng.integers(2, 6))
        cuts = sorted(rng.choice(np.arange(4, total - 4), size=n_seg - 1, replace=False).tolist())
        edges = [0] + cuts + [total]
        segs = []
        for qs, qe in zip(edges[:-1], edges[1:]):
            overlap = int(rng.integers(0, 3)) if qs > 0 and rng.random() < 0.3 else 0
            qs -= overlap
            gap = int(rng.integers(0, 6)) if rng.random() < 0.3 else 0
            qe = max(qs + 1, qe - gap)
            contig = CONTIGS[0] if rng.random() < 0.8 else str(rng.choice(CONTIGS[1:] + ("chrQ",)))
            strand = int(rng.random() < 0.3)
            near = int(rng.integers(80, FUZZ_LENGTH - 80)) if not segs or rng.random() < 0.4 else segs[-1][2] + int(rng.integers(-40, 60))
            near = min(max(near, 0), FUZZ_LENGTH - (qe - qs) - 1)
            segs.append((contig, strand, near, qs, qe, int(rng.choice([60, 60, 60, 9, 10]))))
        primary = int(rng.integers(len(segs)))
        segs[primary] = (CONTIGS[0],) + segs[primary][1:]

        def cigar_of(seg, letter="S"):
            _, strand, _, qs, qe, _ = seg
            lead, trail = (total - qe, qs) if strand else (qs, total - qe)
            return [(letter, lead)] * (lead > 0) + [("M", qe - qs)] + [(letter, trail)] * (trail > 0)

        order = [i for i in rng.permutation(len(segs)) if i != primary]
        tag = b"".join(sa(segs[i][0], segs[i][2], "+-"[segs[i][1]], "".join("%d%s" % (n, op) for op, n in cigar_of(segs[i], "SH"[int(rng.integers(2))])),
                          segs[i][5], int(rng.integers(0, 30))) for i in order)
        if rng.random() < 0.25:
            text = bytearray(tag)
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(len(text)))
                how = int(rng.integers(3))
                byte = int(rng.choice(list(b";,+-0123456789MIDNSHP=Xc\x00\xff")))
                if how == 0:
                    text[at] = byte
                elif how == 1:
                    text.insert(at, byte)
                elif len(text) > 1:
                    del text[at]
            tag = bytes(text)
        _, strand, pos, _, _, mapq = segs[primary]
        cigar = [("MIDNSHP=X".index(op), n) for op, n in cigar_of(segs[primary])]
        rows.append(tagged(sc.row(name, reference, pos, cigar, REV * strand, mapq, int(rng.integers(3))), tag))
    for s in range(0, FUZZ_LENGTH - 120, 61):                 # plain reads for the depth
        rows.append(tagged(sc.row(100 + s, reference, s, [(M, 120)])))
    rows.sort(key=lambda r: r[2])
    return reference, rows
