"""Writes tests/golden/pacbio_clip_cases.json: reads, clip positions and flanks, and what the reference's own
PileupContainerLite.strictClipRead makes of them.  The tests read only the JSON.

    python tests/golden/make_pacbio_clip_fixture.py /path/to/reference/python

The reference's module is imported at generation time only, with a stand-in ``pysam`` module (the two clip functions never touch
it).  A case: ``pos``, ``cigar`` [[op, length]], ``seq``, ``qual`` (phred + 33 text), ``flank`` and ``steps`` [[position, left]]
applied in order to one copy of the read; ``out``: reference_start, reference_end, cigartuples, query_sequence and
query_qualities afterwards.  The hand cases come first, then seeded random CIGARs over M I D N S H = X.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
QUERY, REF = (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)


def hand_cases():
    """(name, pos, cigar, flank, steps)."""
    return [
        ("left then right, flank 200", 1000, [(0, 300), (1, 2), (0, 300)], 200, [(1290, True), (1400, False)]),
        ("inside an M", 100, [(0, 60)], 10, [(130, True)]),
        ("inside an M, right", 100, [(0, 60)], 10, [(130, False)]),
        ("inside a D", 100, [(0, 20), (2, 10), (0, 30)], 5, [(124, True)]),
        ("inside a D, right", 100, [(0, 20), (2, 10), (0, 30)], 5, [(124, False)]),
        ("inside an N", 100, [(0, 20), (3, 10), (0, 30)], 5, [(125, True)]),
        ("inside an N, right", 100, [(0, 20), (3, 10), (0, 30)], 5, [(125, False)]),
        ("at the first aligned base", 100, [(0, 40)], 5, [(100, True)]),
        ("at the first aligned base, right", 100, [(0, 40)], 5, [(100, False)]),
        ("at the last aligned base", 100, [(0, 40)], 5, [(139, True)]),
        ("at the last aligned base, right", 100, [(0, 40)], 5, [(139, False)]),
        ("left of the read", 100, [(0, 40)], 5, [(99, True), (99, False)]),
        ("right of the read", 100, [(0, 40)], 5, [(140, True), (140, False)]),
        ("flank longer than the read", 100, [(0, 40)], 200, [(120, True), (125, False)]),
        ("leading I to S, truncated", 100, [(0, 10), (1, 6), (0, 30)], 8, [(114, True)]),
        ("leading I to S, not truncated", 100, [(1, 4), (0, 30)], 50, [(110, True)]),
        ("trailing I to S, truncated", 100, [(0, 30), (1, 6), (0, 10)], 8, [(124, False)]),
        ("trailing I to S, not truncated", 100, [(0, 30), (1, 4)], 50, [(110, False)]),
        ("a right half that is only an I", 100, [(0, 30), (1, 4)], 50, [(129, False)]),
        ("soft clips count as read bases", 100, [(4, 6), (0, 30), (4, 6)], 12, [(109, True), (120, False)]),
        ("soft clip partly kept", 100, [(4, 6), (0, 10)], 12, [(109, True)]),
        ("centre merged", 100, [(0, 20), (1, 3), (0, 20)], 4, [(110, True)]),
        ("centre not merged", 100, [(0, 20), (1, 3), (0, 20)], 4, [(119, True)]),
        ("centre not merged, right", 100, [(0, 20), (2, 3), (0, 20)], 4, [(119, False)]),
        ("adjacent equal operations merge at the centre", 100, [(0, 20), (0, 20)], 4, [(119, True)]),
        ("hard clips", 100, [(5, 7), (0, 30), (5, 9)], 50, [(110, True), (120, False)]),
        ("hard clips discarded", 100, [(5, 7), (0, 30), (5, 9)], 3, [(110, True), (120, False)]),
        ("deletions on the way out", 100, [(0, 5), (2, 3), (0, 5), (2, 2), (0, 10), (2, 4), (0, 5), (2, 1), (0, 5)], 6, [(114, True), (116, False)]),
        ("= and X", 100, [(7, 10), (8, 2), (7, 20), (8, 1), (7, 10)], 9, [(115, True), (125, False)]),
        ("left and right in one operation", 100, [(0, 1000)], 200, [(500, True), (530, False)]),
    ]


def random_cases(rng, n):
    out = []
    for i in range(n):
        long_read = i % 5 == 0
        flank = 200 if long_read else int(rng.integers(0, 40))
        target = int(rng.integers(300, 700)) if long_read else int(rng.integers(5, 160))
        cigar, total = [], 0
        if rng.random() < 0.2:
            cigar.append((5, int(rng.integers(1, 9))))
        if rng.random() < 0.3:
            cigar.append((4, int(rng.integers(1, 12))))
        while total < target:
            op = int(rng.choice([0, 0, 0, 1, 2, 3, 7, 8, 4, 5], p=[0.3, 0.1, 0.1, 0.15, 0.12, 0.05, 0.08, 0.06, 0.02, 0.02]))
            length = int(rng.integers(1, 60 if op in (0, 7) else 9))
            cigar.append((op, length))
            total += length if op in QUERY else 0
        if rng.random() < 0.3:
            cigar.append((4, int(rng.integers(1, 12))))
        if rng.random() < 0.2:
            cigar.append((5, int(rng.integers(1, 9))))
        pos = int(rng.integers(50, 5000))
        rlen = sum(k for op, k in cigar if op in REF)
        a = pos + int(rng.integers(-3, rlen + 3))
        span = int(rng.integers(1, 200))
        steps = [(a, True), (a + span, False)]
        if i % 7 == 3:
            steps = [(a, False)]
        if i % 7 == 5:
            steps = [(a, True)]
        out.append((f"random {i}", pos, cigar, flank, steps))
    return out


def main(reference_python):
    sys.path.insert(0, reference_python)
    sys.modules.setdefault("pysam", types.ModuleType("pysam"))
    import PileupContainerLite as pcl
    rng = np.random.default_rng(20261017)
    cases = []
    for name, pos, cigar, flank, steps in hand_cases() + random_cases(rng, 260):
        qlen = sum(k for op, k in cigar if op in QUERY)
        rlen = sum(k for op, k in cigar if op in REF)
        seq = "".join(rng.choice(list("ACGT"), size=qlen)) if qlen else ""
        qual = [int(q) for q in rng.integers(2, 42, size=qlen)]
        lead = sum(k for op, k in cigar[:next((i for i, (op, _) in enumerate(cigar) if op not in (4, 5)), len(cigar))] if op == 4)
        trail = 0
        for op, k in reversed(cigar):
            if op not in (4, 5):
                break
            trail += k if op == 4 else 0
        segment = pcl.AlignedSegmentFunctional(pos, pos + max(rlen, 1), [tuple(c) for c in cigar], seq, list(qual),
                                               seq[lead:qlen - trail], list(qual[lead:qlen - trail]), name, False, 60)
        read = pcl.PileupReadDummy(segment)
        for position, left in steps:
            pcl.strictClipRead(read, position, left=left, flankLength=flank)
        s = read.alignment
        text = lambda q: "".join(chr(33 + int(v)) for v in q)  # noqa: E731
        cases.append({"name": name, "pos": pos, "cigar": [list(c) for c in cigar], "seq": seq, "qual": text(qual), "flank": flank,
                      "steps": [[p, bool(left)] for p, left in steps],
                      "out": {"pos": int(s.reference_start), "end": int(s.reference_end), "cigar": [[int(o), int(k)] for o, k in s.cigartuples],
                              "seq": s.query_sequence, "qual": text(s.query_qualities)}})
    path = os.path.join(HERE, "pacbio_clip_cases.json")
    with open(path, "w") as fh:
        json.dump(cases, fh, separators=(",", ":"))
        fh.write("\n")
    print(path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
