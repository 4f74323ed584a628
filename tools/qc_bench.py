"""Quality-metrics benchmark on the synthetic chromosome of tools/refblocks_bench.py: the Illumina reads joined into pairs as
tools/phase_bench.py --paired joins them; the pass (hello_amd/qc.py: measure) split into BAM decode, the four kernel times (HIP
events), the rest of the library's calls (the host's walk and planning, uploads, copies back) and the whole pass.  Beside them
``hello_refblocks_find``'s kernel time on the same reads -- the yardstick: the depth kernel does a subset of its count launch's
work, the reads kernel visits the same bases -- and the two ratios.

    python tools/qc_bench.py [--length 1000000] [--coverage 30] [--read-length 150] [--quality-bins 0] [--repeats 3] [--profile FILE]

``--quality-bins N`` (4 or 8) maps the qualities onto N values, as Illumina instruments report them: what the QUALITY table's adds
meet.  One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the maximum of each time
and, with --profile, appends it to FILE."""
import argparse
import dataclasses
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.bam_writer import write_bam  # noqa: E402
from tools.candidates_bench import spread  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402
from tools.phase_bench import join_pairs  # noqa: E402
from tools.refblocks_bench import emit  # noqa: E402

KERNELS = ("reads_ms", "depth_ms", "pair_ms", "insert_ms")


def binned(reads, bins):
    """Every quality replaced by the centre of its bin of [20, 41), the range tools/hotspot_bench.py synthesises."""
    width = 21 // bins
    table = np.array([20 + min(max(q - 20, 0) // width, bins - 1) * width + width // 2 for q in range(256)], np.uint8)
    as_array = lambda q: np.frombuffer(q, np.uint8) if isinstance(q, (bytes, bytearray)) else np.asarray(q, np.uint8)   # noqa: E731
    return [dataclasses.replace(r, qual=table[as_array(r.qual)].tobytes()) for r in reads]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--insert", type=int, default=450, help="from the first mate's start to the second mate's end")
    ap.add_argument("--quality-bins", type=int, default=0, help="map the qualities onto this many values (0: as synthesised)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    from hello_amd import gvcf, qc
    from hello_amd.bam import BamFile

    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    reads = join_pairs(reads, args.insert, args.coverage, args.read_length)
    if args.quality_bins:
        reads = binned(reads, args.quality_bins)
    names = ("bam_decode_s",) + KERNELS + ("library_calls_s", "host_plan_upload_copy_s", "pass_s", "refblocks_kernel_ms")
    times = {k: [] for k in names}
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "pairs.bam")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with BamFile(bam) as b:
            decoded = b.fetch("chr1", 0, len(ref))
        metrics = None
        for i in range(args.repeats + 1):
            st: dict = {}
            metrics = qc.measure(bam, {"chr1": ref}, ["chr1"], stats=st)
            _, rst, _ = gvcf.find_blocks([decoded], ref, 0, len(ref))
            if i == 0:
                continue                                            # warm-up: library load, first launches
            kernels_s = sum(st[k] for k in KERNELS) / 1e3
            for k, v in (("bam_decode_s", st["decode_s"]), ("library_calls_s", st["device_s"]),
                         ("host_plan_upload_copy_s", st["device_s"] - kernels_s), ("pass_s", st["total_s"]),
                         ("refblocks_kernel_ms", rst["kernel_ms"])) + tuple((k, st[k]) for k in KERNELS):
                times[k].append(v)
    total = metrics.total()
    yardstick = min(times["refblocks_kernel_ms"])
    out = {"qc": "illumina pairs", "length": args.length, "reads": len(reads), "quality_bins": args.quality_bins,
           "distinct_qualities": int((total["QUALITY"][:, 0] > 0).sum()), "repeats": args.repeats,
           "measured": int(total["STATS"][0]), "pairs": int(total["STATS"][4]), "mean_depth": round(metrics.summary()["mean_depth"], 3),
           "library": os.environ.get("HELLO_LIB", "in-tree"),
           "reads_over_refblocks": round(min(times["reads_ms"]) / yardstick, 4),
           "depth_over_refblocks": round(min(times["depth_ms"]) / yardstick, 4)}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
