"""Candidate stage benchmark on the synthetic chromosome of tools/hotspot_bench.py: hotspot positions -> candidate sites timed
end to end (BAM decode included) and split into BAM decode, the three kernels (HIP events), the host gather and the rest of
the call (planning, transfers), plus the CPU restatement (tests/candidate_reference.py) on a slice for context.

    python tools/candidates_bench.py [--length 5000000] [--coverage 30] [--read-length 150] [--slice 20000] [--repeats 5] [--pacbio]

--pacbio: the reads are treated as PacBio reads (give a --read-length of several thousand): PacBio hotspots, the read cap of 100
per 100 bp, strict clipping -- the two clip kernels are timed with the other stages (clip_kernel_ms).

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the spread of each time."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import candidate_reference as cr  # noqa: E402
from tests import pacbio_reference as pr  # noqa: E402
from tests.bam_writer import write_bam  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402


def spread(values):
    v = np.asarray(values, float)
    return {"min": round(float(v.min()), 4), "median": round(float(np.median(v)), 4), "max": round(float(v.max()), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--slice", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pacbio", action="store_true", default=False, help="PacBio reads: read cap, strict clipping, the clip kernels' time")
    args = ap.parse_args()
    from hello_amd import candidates as cd, hotspots as hs
    from hello_amd.bam import BamFile

    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "x.bam")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with BamFile(bam) as b:
            r = b.fetch("chr1", 0, len(ref))
        positions, _ = hs.find_positions([r], ref, [(0, len(ref))], pacbio=args.pacbio)
        times = {k: [] for k in ("end_to_end_s", "bam_decode_s", "call_s", "pass1_kernel_ms", "pass2_kernel_ms", "allele_kernel_ms",
                                 "clip_kernel_ms", "gather_ms", "call_rest_ms")}
        st = {}
        for i in range(args.repeats + 1):
            t0 = time.perf_counter()
            with BamFile(bam) as b:
                r = b.fetch("chr1", 0, len(ref))
            t1 = time.perf_counter()
            shard, st, _ = cd.find_sites(r, ref, positions, "chr1", options=hs.HOTSPOTS_PACBIO if args.pacbio else 0)
            t2 = time.perf_counter()
            if i == 0:
                continue                                          # warm-up: library load, first launches
            kernels = st["pass1_kernel_ms"] + st["pass2_kernel_ms"] + st["allele_kernel_ms"] + st["clip_kernel_ms"]
            for k, v in (("end_to_end_s", t2 - t0), ("bam_decode_s", t1 - t0), ("call_s", t2 - t1),
                         ("call_rest_ms", st["total_ms"] - kernels - st["gather_ms"])):
                times[k].append(v)
            for k in ("pass1_kernel_ms", "pass2_kernel_ms", "allele_kernel_ms", "clip_kernel_ms", "gather_ms"):
                times[k].append(st[k])
        a = len(ref) // 2
        sl = [x for x in reads if x.pos < a + args.slice + 200 and x.ref_end > a - 200]
        sl_pos = [int(p) for p in positions if a <= p < a + args.slice]
        t = time.perf_counter()
        want = (pr if args.pacbio else cr).find_candidates(sl, ref, sl_pos)
        t_cpu = time.perf_counter() - t
    sites = int(st["sites"])
    out = {"pacbio": bool(args.pacbio), "reads_clipped": int(st["reads_clipped"]), "length": args.length, "coverage": args.coverage, "reads": len(reads), "positions": int(len(positions)), "sites": sites,
           "alleles": int(st["alleles"]), "reads_gathered": int(st["reads_gathered"]), "record_slots": int(st["record_slots"]),
           "active_regions": int(st["active_regions"]), "clusters": int(st["clusters"]), "repeats": args.repeats,
           "sites_per_s_end_to_end": round(sites / min(times["end_to_end_s"])),
           "sites_per_s_without_bam_decode": round(sites / min(times["call_s"])),
           "slice_bp": args.slice, "slice_sites": len(want), "slice_cpu_restatement_s": round(t_cpu, 3),
           "cpu_restatement_sites_per_s": round(len(want) / max(t_cpu, 1e-9), 1)}
    out.update({k: spread(v) for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
