"""Pileup-at-sites benchmark on the synthetic chromosome of tools/refblocks_bench.py: 30x of reads of --read-length bases (150:
Illumina-like; 15000: HiFi-like), sites at one position in 300 and one in 3 000.  The pass (hello_amd/contamination.py: measure)
split into BAM decode, the two kernel times (HIP events: the sites kernels once per chromosome, the reads kernel per span) in both
forms of the reads kernel -- two phases, and plain -- the rest of the library's calls, the whole pass and the estimator's host time
at the benchmark's site count.  Beside them ``hello_refblocks_find``'s kernel time on the same reads -- the yardstick of sections
7j, 7k and 7m -- and the ratios.

    python tools/pileup_bench.py [--length 1000000] [--coverage 30] [--read-length 150] [--share 0] [--repeats 3] [--profile FILE]

--share: the counting reads of a workgroup of the reads kernel (0: every launch sizes it, the default of the library).

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the maximum of each time and,
with --profile, appends it to FILE."""
import argparse
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
from tools.refblocks_bench import emit  # noqa: E402

DENSITIES = (300, 3000)
FORMS = (("two_phase", 0), ("plain", 1))


def sites_at(ref: str, one_in: int, seed: int):
    """A ``contamination.Sites`` of about len(ref) / one_in random positions of ``chr1`` with a random ALT and AF."""
    from hello_amd import contamination as cn
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(len(ref), size=len(ref) // one_in, replace=False)).astype(np.int64)
    codes = cn._CODE[np.frombuffer(ref.encode(), np.uint8)[pos]]
    keep = codes < 4
    pos, codes = pos[keep], codes[keep]
    sites = cn.Sites(["chr1"])
    sites.per_chromosome["chr1"] = dict(POS=pos, REF=codes, ALT=((codes + rng.integers(1, 4, size=pos.shape[0])) % 4).astype(np.uint8),
                                        AF=rng.uniform(0.05, 0.95, size=pos.shape[0]))
    sites.records = int(pos.shape[0])
    return sites


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--share", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    from hello_amd import contamination as cn, gvcf
    from hello_amd.bam import BamFile

    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    ref = ref if isinstance(ref, str) else bytes(ref).decode()
    site_sets = {d: sites_at(ref, d, 11 + d) for d in DENSITIES}
    names = ["bam_decode_s", "refblocks_kernel_ms"]
    for d in DENSITIES:
        names += ["sites_ms_1in%d" % d, "estimate_s_1in%d" % d] + ["%s_%s_1in%d" % (k, f, d) for f, _ in FORMS for k in ("reads_ms", "library_calls_s", "pass_s")]
    times = {k: [] for k in names}
    found, tables = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "reads.bam")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        for i in range(args.repeats + 1):
            with BamFile(bam) as b:
                t0 = time.perf_counter()
                decoded = b.fetch("chr1", 0, len(ref))
                t1 = time.perf_counter()
            row = {"bam_decode_s": t1 - t0}
            for d in DENSITIES:
                for form, code in FORMS:
                    st: dict = {}
                    found[d] = cn.measure(bam, {"chr1": ref}, ["chr1"], site_sets[d], stats=st, form=code, share=args.share)
                    tables[(d, form)] = found[d].tables["chr1"]["COUNTS"].tobytes()
                    row.update({"reads_ms_%s_1in%d" % (form, d): st["reads_ms"], "library_calls_s_%s_1in%d" % (form, d): st["device_s"],
                                "pass_s_%s_1in%d" % (form, d): st["total_s"], "sites_ms_1in%d" % d: st["sites_ms"]})
                t0 = time.perf_counter()
                found[d].estimate()
                row["estimate_s_1in%d" % d] = time.perf_counter() - t0
            _, rst, _ = gvcf.find_blocks([decoded], ref, 0, len(ref))
            row["refblocks_kernel_ms"] = rst["kernel_ms"]
            if i == 0:
                continue                                            # warm-up: library load, first launches
            for k, v in row.items():
                times[k].append(v)
    yardstick = min(times["refblocks_kernel_ms"])
    out = {"pileup": "reads of %d" % args.read_length, "length": args.length, "reads": len(reads), "read_length": args.read_length, "share": args.share,
           "repeats": args.repeats, "library": os.environ.get("HELLO_LIB", "in-tree")}
    for d in DENSITIES:
        total = found[d].total()
        out.update({"sites_1in%d" % d: total["n_sites"], "reads_on_a_site_1in%d" % d: total["reads_on_a_site"],
                    "observations_1in%d" % d: total["observations"], "counting": total["counting"],
                    "forms_give_equal_bytes_1in%d" % d: tables[(d, "two_phase")] == tables[(d, "plain")]})
        for form, _ in FORMS:
            out["reads_%s_over_refblocks_1in%d" % (form, d)] = round(min(times["reads_ms_%s_1in%d" % (form, d)]) / yardstick, 4)
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
