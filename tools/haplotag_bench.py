"""Haplotag benchmark on the inputs of tools/phase_bench.py: the fused launch of ``hello_haplotag_reads`` beside ``observe_ms +
tag_ms`` of ``hello_phase_*`` on the same reads and records -- the yardstick: those two launches do the same walk and the same
count, with a slot array between them.

    python tools/haplotag_bench.py [--kinds illumina,pacbio,hybrid] [--length 1000000] [--repeats 3] [--profile FILE]

The 1 Mb synthetic chromosome, 1 000 heterozygous records (one per --record-every bases) and the three read sets of
tools/phase_bench.py.  The records are phased once, from the long reads (150-base reads alone link no two records 1 kb apart),
by ``hello_phase_*`` -- the kernels tests/test_gpu_phase.py holds to the restatement, which itself takes minutes on 200 k reads --
written as phased lines and read back through ``haplotag.phased``.  Per kind the yardstick is ``hello_phase_observe`` over the
kind's reads and ``hello_phase_tag`` with that phasing; the tags of the fused launch must equal its tags before anything is timed.
One warm-up call, then --repeats timed calls on ONE handle (the table is uploaded once, by ``table_upload_ms``); per kind one JSON
line with the minimum, the median and the maximum of each time.  ``transfer_ms`` is what is left of a call beside the plan and the
kernel: the upload of the read set, the allocations and the download of hp / ps; ``tag_wall_ms`` is the whole ``Haplotagger.tag``
call (with two read sets it joins them first, in NumPy)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.bam_writer import write_bam  # noqa: E402
from tools.candidates_bench import pacbio_noise, spread  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402
from tools.refblocks_bench import emit  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--kinds", default="illumina,pacbio,hybrid")
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--pacbio-coverage", type=float, default=25)
    ap.add_argument("--pacbio-read-length", type=int, default=3000)
    ap.add_argument("--record-every", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", help="append the JSON lines to this file")
    args = ap.parse_args()
    from hello_amd import haplotag as ht, phase
    from hello_amd.bam import BamFile

    ref, short = synthesize(args.length, args.coverage, args.read_length)
    _, long_reads = synthesize(args.length, args.pacbio_coverage, args.pacbio_read_length)            # the same seed: the same donor
    noise = np.random.default_rng(7)
    long_reads = [pacbio_noise(r, noise) for r in long_reads]
    lines = [("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t0/1\n" % (p + 1, ref[p], "A" if ref[p] != "A" else "C")).encode()
             for p in range(args.record_every // 2, len(ref), args.record_every)]
    records = [phase.phasable(line) for line in lines]
    decoded = {}
    with tempfile.TemporaryDirectory() as d:
        for name, reads in (("illumina", short), ("pacbio", long_reads)):
            path = os.path.join(d, name + ".bam")
            write_bam(path, [("chr1", len(ref))], reads, index=True)
            with BamFile(path) as b:
                decoded[name] = b.fetch("chr1", 0, len(ref))
    # one phasing for all three kinds, from the long reads: 150-base reads alone link no two records that lie 1 kb apart
    details: dict = {}
    phase.find_haplotags([decoded["pacbio"]], records, details=details)
    sets_of, flips = details["set"], details["flip"]
    set_pos = phase.set_positions(sets_of, [r.pos for r in records])
    back = [ht.phased(phase.phased_line(line, rec, int(f), int(p))) for line, rec, f, p in zip(lines, records, flips, set_pos) if p]
    for kind in args.kinds.split(","):
        sets = [decoded["illumina"], decoded["pacbio"]] if kind == "hybrid" else [decoded[kind]]
        names = ("phase_plan_ms", "phase_observe_ms", "phase_link_ms", "phase_tag_ms", "phase_observe_plus_tag_ms", "fused_kernel_ms",
                 "plan_ms", "transfer_ms", "call_ms", "tag_wall_ms")
        times = {k: [] for k in names}
        for i in range(args.repeats + 1):                           # the yardstick: observe, then tag with that phasing
            with phase.Phaser(records) as ph:
                ph.observe(sets)
                want = ph.tag(sets_of, flips)
                st = ph.stats()
            if i:
                for k in ("plan", "observe", "link", "tag"):
                    times["phase_%s_ms" % k].append(st[k + "_ms"])
                times["phase_observe_plus_tag_ms"].append(st["observe_ms"] + st["tag_ms"])
        with ht.Haplotagger(None, records={"chr1": back}) as tagger:
            t0 = time.perf_counter()
            tagger._handle("chr1")
            upload = (time.perf_counter() - t0) * 1e3
            before = tagger.stats
            for i in range(args.repeats + 1):
                t0 = time.perf_counter()
                got = tagger.tag("chr1", sets)
                wall = (time.perf_counter() - t0) * 1e3
                after = tagger.stats
                if i == 0 and not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                    raise SystemExit(f"{kind}: the fused launch and the phasing kernels disagree")
                if i:
                    kernel, plan, call = (after[k] - before[k] for k in ("kernel_ms", "plan_ms", "total_ms"))
                    for k, v in (("fused_kernel_ms", kernel), ("plan_ms", plan), ("transfer_ms", call - plan - kernel), ("call_ms", call),
                                 ("tag_wall_ms", wall)):
                        times[k].append(v)
                before = after
        out = {"haplotag": kind, "length": args.length, "reads": [s.n_reads for s in sets], "reads_counted": int(st["reads_counted"]),
               "records": len(records), "phased_records": len(back), "slots": int(st["slots"]),
               "tagged": [int((got[0] == v).sum()) for v in (1, 2, 0)], "repeats": args.repeats, "table_upload_ms": round(upload, 4),
               "fused_over_observe_plus_tag": round(min(times["fused_kernel_ms"]) / min(times["phase_observe_plus_tag_ms"]), 3)}
        out.update({k: spread(v) for k, v in times.items()})
        emit(out, args)


if __name__ == "__main__":
    main()
