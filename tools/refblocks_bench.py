"""Reference-confidence block benchmark on the synthetic chromosome of tools/hotspot_bench.py: the gVCF pass (hello_amd/gvcf.py)
split into BAM decode, plan, the two kernel launches (HIP events), the rest of the call with its host join, and the file write, with
the base visits per second of the kernels; beside it ``hotspot_kernel``'s time on the same reads and span -- the yardstick: it
walks the same bases and keeps more per position.

    python tools/refblocks_bench.py [--length 1000000] [--coverage 30] [--read-length 150] [--repeats 3] [--profile FILE]
    python tools/refblocks_bench.py --pacbio [--pacbio-coverage 25] [--pacbio-read-length 3000]
    python tools/refblocks_bench.py --hybrid
    python tools/refblocks_bench.py --call [--call-length 200000]

--pacbio: one BAM of long reads with PacBio-like indel errors; --hybrid: the Illumina and the PacBio BAM together (source 0 / 1).
--call: wall seconds of ``python -m hello_amd.call --from_bam`` with and without --gvcf on one synthetic chromosome, three
interleaved runs, each a child process under its own time limit.

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the maximum of each time and, with
--profile, appends it to FILE."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.bam_writer import write_bam  # noqa: E402
from tools.candidates_bench import pacbio_noise, spread  # noqa: E402
from tools.hotspot_bench import synthesize  # noqa: E402


def base_visits(sets, mapq_threshold=10):
    """M / = / X / D positions of the counted reads: what the kernel's lanes visit (each once per tile the operation touches)."""
    from hello_amd import gvcf
    total = 0
    for r in sets:
        keep = np.array([gvcf.counted(int(f), int(m), mapq_threshold) for f, m in zip(r.flags, r.mapq)], bool)
        op, n = r.cigars & 15, (r.cigars >> 4).astype(np.int64)
        per_op = np.where(np.isin(op, (0, 2, 7, 8)), n, 0)
        per_read = np.add.reduceat(np.concatenate([per_op, [0]]), np.minimum(r.cigar_offsets[:-1], per_op.shape[0]))
        per_read[np.diff(r.cigar_offsets) == 0] = 0
        total += int(per_read[keep].sum())
    return total


def emit(out, args):
    line = json.dumps(out)
    print(line, flush=True)
    if args.profile:
        with open(args.profile, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pacbio", action="store_true", default=False)
    ap.add_argument("--hybrid", action="store_true", default=False)
    ap.add_argument("--pacbio-coverage", type=float, default=25)
    ap.add_argument("--pacbio-read-length", type=int, default=3000)
    ap.add_argument("--call", action="store_true", default=False, help="wall time of call --from_bam with and without --gvcf")
    ap.add_argument("--call-length", type=int, default=200_000)
    ap.add_argument("--step-timeout", type=int, default=420, help="--call: seconds each child process may take")
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    if args.call:
        return call_wall(args)
    from hello_amd import gvcf, hotspots as hs
    from hello_amd.bam import BamFile

    sets = []
    if not args.pacbio:
        ref, reads = synthesize(args.length, args.coverage, args.read_length)
        sets.append(reads)
    if args.pacbio or args.hybrid:
        ref, long_reads = synthesize(args.length, args.pacbio_coverage, args.pacbio_read_length)      # the same seed: the same donor
        noise = np.random.default_rng(7)
        sets.append([pacbio_noise(r, noise) for r in long_reads])
    names = ("bam_decode_s", "plan_ms", "kernel_ms", "call_rest_ms", "file_write_s", "pass_s", "hotspot_kernel_ms")
    times = {k: [] for k in names}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, rs in enumerate(sets):
            paths.append(os.path.join(d, f"{i}.bam"))
            write_bam(paths[-1], [("chr1", len(ref))], rs, index=True)
        vcf = os.path.join(d, "results.output.vcf")
        with open(vcf, "w") as fh:                                  # a record every 1 000 bases: the excluded intervals of a real run
            fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n")
            for p in range(500, len(ref), 1000):
                fh.write("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t0/1\n" % (p + 1, ref[p], "A" if ref[p] != "A" else "C"))
        decoded = []
        for path in paths:
            with BamFile(path) as b:
                decoded.append(b.fetch("chr1", 0, len(ref)))
        visits = base_visits(decoded)
        blocks = 0
        for i in range(args.repeats + 1):
            st: dict = {}
            t0 = time.perf_counter()
            gvcf.write_gvcf(vcf, paths, {"chr1": ref}, os.path.join(d, "out.g.vcf"), stats=st)
            wall = time.perf_counter() - t0
            _, hst = hs.find_positions(decoded, ref, [(0, len(ref))], pacbio=args.pacbio and not args.hybrid)
            if i == 0:
                continue                                            # warm-up: library load, first launches
            blocks = int(st["blocks"])
            for k, v in (("bam_decode_s", st["decode_s"]), ("plan_ms", st["plan_ms"]), ("kernel_ms", st["kernel_ms"]),
                         ("call_rest_ms", st["total_ms"] - st["plan_ms"] - st["kernel_ms"] + 1e3 * st["join_s"]),
                         ("file_write_s", st["write_s"]), ("pass_s", wall), ("hotspot_kernel_ms", hst["kernel_ms"])):
                times[k].append(v)
    out = {"refblocks": "hybrid" if args.hybrid else "pacbio" if args.pacbio else "illumina", "length": args.length,
           "reads": [len(s) for s in sets], "base_visits": visits, "blocks": blocks, "repeats": args.repeats,
           "base_visits_per_s_in_kernels": round(visits / (min(times["kernel_ms"]) * 1e-3)),
           "base_visits_per_s_whole_pass": round(visits / min(times["pass_s"]))}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


def call_wall(args):
    from hello_amd import loader, netspec as ns, weights
    ref, reads = synthesize(args.call_length, args.coverage, args.read_length)
    times = {"plain_s": [], "gvcf_s": []}
    with tempfile.TemporaryDirectory() as d:
        bam, fa, model = os.path.join(d, "x.bam"), os.path.join(d, "g.fa"), os.path.join(d, "model.hello.npz")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with open(fa, "w") as fh:
            fh.write(">chr1\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))
        vcfs, lines = {}, 0
        for i in range(3):
            for key, extra in (("plain_s", []), ("gvcf_s", ["--gvcf"])):
                work = os.path.join(d, f"{key}{i}")
                t0 = time.perf_counter()
                done = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, "-m", "hello_amd.call", "--ibam", bam,
                                       "--ref", fa, "--workdir", work, "--network", model, "--from_bam"] + extra, cwd=ROOT,
                                      capture_output=True, text=True)
                times[key].append(time.perf_counter() - t0)
                if done.returncode != 0:
                    sys.stderr.write(done.stderr[-3000:])
                    raise SystemExit(f"call {key} ended with status {done.returncode}: nothing further is started")
                vcfs[key] = open(os.path.join(work, "results.output.vcf"), "rb").read()
                if extra:
                    lines = sum(1 for line in open(os.path.join(work, "results.output.g.vcf")) if "<NON_REF>" in line)
        assert vcfs["plain_s"] == vcfs["gvcf_s"]
    out = {"refblocks": "call --from_bam", "length": args.call_length, "reads": len(reads), "blocks": lines,
           "records": sum(1 for line in vcfs["gvcf_s"].splitlines() if not line.startswith(b"#"))}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
