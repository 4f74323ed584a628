"""Duplicate-marking benchmark on the synthetic chromosome of tools/refblocks_bench.py: the Illumina reads joined into pairs as
tools/phase_bench.py --paired joins them, a copy of other qualities planted for one pair in ten; the pass (hello_amd/markdup.py:
find_duplicates) split into BAM decode, the four kernel times (HIP events), the host's gather of the identities and the whole
pass.  Beside the ends kernel ``hello_refblocks_find``'s kernel time on the same reads -- the yardstick: both walk every read and
touch every base, and the ends kernel does less per base -- and the ratio of the two.  Then ``Marks.apply`` inside ``fetch``: the
chromosome fetched in --fetches windows (the candidate stage fetches per shard file, at most 500 a chromosome), the time of the
fetches themselves and of the apply calls on what they return.

    python tools/markdup_bench.py [--length 1000000] [--coverage 30] [--read-length 150] [--duplicates 0.1] [--repeats 3] [--profile FILE]

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the maximum of each time and, with
--profile, appends it to FILE."""
import argparse
import dataclasses
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.bam_writer import write_bam  # noqa: E402
from tools.candidates_bench import spread  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402
from tools.phase_bench import join_pairs  # noqa: E402
from tools.refblocks_bench import emit  # noqa: E402


def plant(reads, fraction, seed=3):
    """A copy of both mates, under another name and at lower qualities, for ``fraction`` of the pairs -> reads sorted by start."""
    rng = np.random.default_rng(seed)
    by_name = {}
    for r in reads:
        if r.flag & 0x1:
            by_name.setdefault(r.name, []).append(r)
    out = list(reads)
    for name, mates in by_name.items():
        if len(mates) == 2 and rng.random() < fraction:
            out += [dataclasses.replace(m, name=name + "_copy", qual=[max(int(x) - 3, 2) for x in m.qual]) for m in mates]
    out.sort(key=lambda r: r.pos)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--insert", type=int, default=450, help="from the first mate's start to the second mate's end")
    ap.add_argument("--duplicates", type=float, default=0.1, help="fraction of the pairs that get a copy")
    ap.add_argument("--fetches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    from hello_amd import gvcf, markdup
    from hello_amd.bam import BamFile

    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    reads = plant(join_pairs(reads, args.insert, args.coverage, args.read_length), args.duplicates)
    names = ("bam_decode_s", "ends_ms", "pair_ms", "key_ms", "mark_ms", "host_gather_s", "pass_s", "refblocks_kernel_ms", "fetch_s", "apply_s")
    times = {k: [] for k in names}
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "pairs.bam")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with BamFile(bam) as b:
            decoded = b.fetch("chr1", 0, len(ref))
        step = -(-len(ref) // args.fetches)
        marks = None
        for i in range(args.repeats + 1):
            st: dict = {}
            marks = markdup.find_duplicates(bam, ["chr1"], stats=st)
            _, rst, _ = gvcf.find_blocks([decoded], ref, 0, len(ref))
            fetch_s = apply_s = 0.0
            with BamFile(bam) as b:
                for lo in range(0, len(ref), step):
                    t0 = time.perf_counter()
                    rd = b.fetch("chr1", lo, min(lo + step, len(ref)))
                    t1 = time.perf_counter()
                    marks.apply("chr1", rd)
                    fetch_s += t1 - t0
                    apply_s += time.perf_counter() - t1
            if i == 0:
                continue                                            # warm-up: library load, first launches
            for k, v in (("bam_decode_s", st["decode_s"]), ("ends_ms", st["ends_ms"]), ("pair_ms", st["pair_ms"]), ("key_ms", st["key_ms"]),
                         ("mark_ms", st["mark_ms"]), ("host_gather_s", st["gather_s"]), ("pass_s", st["total_s"]),
                         ("refblocks_kernel_ms", rst["kernel_ms"]), ("fetch_s", fetch_s), ("apply_s", apply_s)):
                times[k].append(v)
        total = marks.total()
    out = {"markdup": "illumina pairs", "length": args.length, "reads": len(reads), "duplicates_planted": args.duplicates,
           "fetches": args.fetches, "repeats": args.repeats, **total,
           "ends_over_refblocks": round(min(times["ends_ms"]) / min(times["refblocks_kernel_ms"]), 4)}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
