"""Methylation benchmark on the synthetic chromosome of tools/refblocks_bench.py under HiFi-like reads: 15 kb, about 30x, every
CpG of a read listed in its MM / ML tags (the reference's density: one position in sixteen).  The pass (hello_amd/methylation.py:
measure) split into BAM decode with and without the tag parsing, the two kernel times (HIP events: the site kernels once per
chromosome, the reads kernel per span), the rest of the library's calls and the whole pass.  Beside them ``hello_refblocks_find``'s
kernel time on the same reads -- the yardstick of sections 7j and 7k -- and the ratio.

    python tools/methylation_bench.py [--length 1000000] [--coverage 30] [--read-length 15000] [--repeats 3] [--profile FILE]

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the maximum of each time and,
with --profile, appends it to FILE."""
import argparse
import dataclasses
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.bam_writer import write_bam  # noqa: E402
from tools.candidates_bench import spread  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402
from tools.refblocks_bench import emit  # noqa: E402

KERNELS = ("sites_ms", "reads_ms")


def with_calls(read, rng, n):
    """``read`` with the MM / ML tags an instrument writes: every CpG of the read on its own strand, a random probability, and
    for two reads in three an HP tag."""
    b = np.frombuffer(read.seq.encode(), np.uint8)
    reverse = bool(read.flag & 0x10)
    at = np.flatnonzero(b == (ord("G") if reverse else ord("C")))
    if reverse:
        at = at[::-1]
        cpg = (at > 0) & (b[np.maximum(at - 1, 0)] == ord("C"))
    else:
        cpg = (at + 1 < b.shape[0]) & (b[np.minimum(at + 1, b.shape[0] - 1)] == ord("G"))
    ordinals = np.flatnonzero(cpg)
    deltas = np.diff(ordinals, prepend=-1) - 1
    mm = b"C+m?" + b"".join(b",%d" % d for d in deltas.tolist()) + b";"
    ml = rng.integers(0, 256, size=ordinals.shape[0]).astype(np.uint8).tobytes()
    hp = n % 3
    tags = (b"HPC" + bytes([hp]) if hp else b"") + b"MMZ" + mm + b"\0" + b"MLBC" + struct.pack("<I", len(ml)) + ml
    return dataclasses.replace(read, tags=tags), int(ordinals.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=15000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    from hello_amd import gvcf, methylation
    from hello_amd.bam import BamFile

    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    rng = np.random.default_rng(5)
    tagged = [with_calls(r, rng, n) for n, r in enumerate(reads)]
    reads, listed = [t[0] for t in tagged], sum(t[1] for t in tagged)
    names = ("bam_decode_plain_s", "bam_decode_with_mods_s") + KERNELS + ("library_calls_s", "host_plan_upload_copy_s", "pass_s",
                                                                         "refblocks_kernel_ms")
    times = {k: [] for k in names}
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "hifi.bam")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        found = None
        for i in range(args.repeats + 1):
            with BamFile(bam) as b:
                t0 = time.perf_counter()
                decoded = b.fetch("chr1", 0, len(ref))
                t1 = time.perf_counter()
                b.fetch_with_mods("chr1", 0, len(ref))
                t2 = time.perf_counter()
            st: dict = {}
            found = methylation.measure(bam, {"chr1": ref}, ["chr1"], stats=st)
            _, rst, _ = gvcf.find_blocks([decoded], ref, 0, len(ref))
            if i == 0:
                continue                                            # warm-up: library load, first launches
            kernels_s = sum(st[k] for k in KERNELS) / 1e3
            for k, v in (("bam_decode_plain_s", t1 - t0), ("bam_decode_with_mods_s", t2 - t1), ("library_calls_s", st["device_s"]),
                         ("host_plan_upload_copy_s", st["device_s"] - kernels_s), ("pass_s", st["total_s"]),
                         ("refblocks_kernel_ms", rst["kernel_ms"])) + tuple((k, st[k]) for k in KERNELS):
                times[k].append(v)
    total = found.total()
    yardstick = min(times["refblocks_kernel_ms"])
    out = {"methylation": "hifi", "length": args.length, "reads": len(reads), "read_length": args.read_length, "listed_bases": listed,
           "repeats": args.repeats, "sites": total["n_sites"], "counting": total["counting"], "observations": total["observations"],
           "library": os.environ.get("HELLO_LIB", "in-tree"),
           "reads_over_refblocks": round(min(times["reads_ms"]) / yardstick, 4),
           "sites_over_refblocks": round(min(times["sites_ms"]) / yardstick, 4)}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
