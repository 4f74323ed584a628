"""Phasing benchmark on the synthetic chromosome of tools/refblocks_bench.py: the phase pass (hello_amd/phase.py) split into BAM
decode, host plan, the observe, link and tag launches (HIP events), the chain and the file write, with the slots per second of the
kernels; beside it ``hello_refblocks_find``'s kernel time on the same reads -- the yardstick: it walks every CIGAR of every counted
read and visits every base, where the observe launch visits only the bases inside records.

    python tools/phase_bench.py [--length 1000000] [--coverage 30] [--read-length 150] [--repeats 3] [--profile FILE]
    python tools/phase_bench.py --pacbio [--pacbio-coverage 25] [--pacbio-read-length 3000]
    python tools/phase_bench.py --hybrid
    python tools/phase_bench.py --paired [--insert 450] [--record-every 1000]

--paired: the Illumina reads joined into pairs; the pass runs without and with ``fragments=True`` on the same BAM, interleaved,
and the line holds both: the kernels' times (pair, fragment link and fragment tag beside observe, link and tag), the whole pass
and the number of records that get a PS.

Heterozygous records are planted in the VCF at one per --record-every bases (REF: the reference base; the reads are those of one
donor, so most show the a allele: the walk and the slot count are what is timed, not the sets).  One warm-up run, then --repeats
timed runs; prints one JSON line with the minimum, the median and the maximum of each time and, with --profile, appends it to FILE."""
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


def join_pairs(reads, insert, coverage, read_len):
    """The reads (sorted by start) made into pairs whose starts lie about ``insert - read_len`` apart: every other stretch of k
    reads joined with the next stretch, one name per pair, flags 0x43 / 0x83 beside the strand bit."""
    k = max(1, round(coverage / read_len * (insert - read_len)))
    for i in range(0, len(reads) - k):
        if (i // k) % 2 == 0:
            reads[i].name = reads[i + k].name = "p%d" % i
            reads[i].flag |= 0x43
            reads[i + k].flag |= 0x83
    return reads


def paired(args):
    """--paired: the Illumina reads as pairs; the pass without and with --phase_fragments on the same BAM, interleaved."""
    from hello_amd import phase
    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    reads = join_pairs(reads, args.insert, args.coverage, args.read_length)
    names = ("bam_decode_s", "plan_ms", "observe_ms", "link_ms", "tag_ms", "chain_s", "file_write_s", "pass_s")
    extra = ("join_s", "pair_ms", "fragment_link_ms", "fragment_tag_ms")
    times = {False: {k: [] for k in names}, True: {k: [] for k in names + extra}}
    counts = {}
    with tempfile.TemporaryDirectory() as d:
        bam, vcf = os.path.join(d, "pairs.bam"), os.path.join(d, "results.output.vcf")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with open(vcf, "w") as fh:
            fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n")
            for p in range(args.record_every // 2, len(ref), args.record_every):
                fh.write("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t0/1\n" % (p + 1, ref[p], "A" if ref[p] != "A" else "C"))
        for i in range(args.repeats + 1):
            for fragments in (False, True):
                st: dict = {}
                out = os.path.join(d, "out%d.phased.vcf" % fragments)
                t0 = time.perf_counter()
                phase.write_phased_vcf(vcf, [bam], out, stats=st, fragments=fragments)
                wall = time.perf_counter() - t0
                if i == 0:
                    continue                                        # warm-up: library load, first launches
                st.update(bam_decode_s=st["decode_s"], file_write_s=st["write_s"], pass_s=wall)
                for k in times[fragments]:
                    times[fragments][k].append(st[k])
                with open(out, "rb") as fh:
                    with_ps = sum(1 for line in fh if not line.startswith(b"#") and b"|" in line.split(b"\t")[9])
                counts[fragments] = dict(records=int(st["records"]), slots=int(st["slots"]), records_with_ps=with_ps,
                                         pairs=int(st.get("pairs", 0)), groups_refused=int(st.get("groups_refused", 0)))
    out = {"phase": "illumina pairs", "length": args.length, "reads": len(reads), "insert": args.insert,
           "record_every": args.record_every, "repeats": args.repeats}
    for fragments, label in ((False, "per_read"), (True, "fragments")):
        out[label] = dict(counts[fragments], **{k: spread(v) for k, v in times[fragments].items()})
    emit(out, args)


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
    ap.add_argument("--record-every", type=int, default=1000)
    ap.add_argument("--paired", action="store_true", default=False,
                    help="the Illumina reads as pairs: the pass without and with --phase_fragments (DESIGN.md section 7i)")
    ap.add_argument("--insert", type=int, default=450, help="--paired: from the first mate's start to the second mate's end")
    ap.add_argument("--profile", help="append the JSON line to this file")
    args = ap.parse_args()
    if args.paired:
        return paired(args)
    from hello_amd import gvcf, phase
    from hello_amd.bam import BamFile

    sets = []
    if not args.pacbio:
        ref, reads = synthesize(args.length, args.coverage, args.read_length)
        sets.append(reads)
    if args.pacbio or args.hybrid:
        ref, long_reads = synthesize(args.length, args.pacbio_coverage, args.pacbio_read_length)      # the same seed: the same donor
        noise = np.random.default_rng(7)
        sets.append([pacbio_noise(r, noise) for r in long_reads])
    names = ("bam_decode_s", "plan_ms", "observe_ms", "link_ms", "tag_ms", "chain_s", "file_write_s", "pass_s", "refblocks_kernel_ms")
    times = {k: [] for k in names}
    slots = records = 0
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, rs in enumerate(sets):
            paths.append(os.path.join(d, f"{i}.bam"))
            write_bam(paths[-1], [("chr1", len(ref))], rs, index=True)
        vcf = os.path.join(d, "results.output.vcf")
        with open(vcf, "w") as fh:
            fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE1\n")
            for p in range(args.record_every // 2, len(ref), args.record_every):
                fh.write("chr1\t%d\t.\t%s\t%s\t30\t.\tHELLO\tGT\t0/1\n" % (p + 1, ref[p], "A" if ref[p] != "A" else "C"))
        decoded = []
        for path in paths:
            with BamFile(path) as b:
                decoded.append(b.fetch("chr1", 0, len(ref)))
        for i in range(args.repeats + 1):
            st: dict = {}
            t0 = time.perf_counter()
            phase.write_phased_vcf(vcf, paths, os.path.join(d, "out.phased.vcf"), stats=st)
            wall = time.perf_counter() - t0
            _, rst, _ = gvcf.find_blocks(decoded, ref, 0, len(ref))
            if i == 0:
                continue                                            # warm-up: library load, first launches
            slots, records = int(st["slots"]), int(st["records"])
            for k, v in (("bam_decode_s", st["decode_s"]), ("plan_ms", st["plan_ms"]), ("observe_ms", st["observe_ms"]),
                         ("link_ms", st["link_ms"]), ("tag_ms", st["tag_ms"]), ("chain_s", st["chain_s"]), ("file_write_s", st["write_s"]),
                         ("pass_s", wall), ("refblocks_kernel_ms", rst["kernel_ms"])):
                times[k].append(v)
    kernels = min(times["observe_ms"]) + min(times["link_ms"]) + min(times["tag_ms"])
    out = {"phase": "hybrid" if args.hybrid else "pacbio" if args.pacbio else "illumina", "length": args.length,
           "reads": [len(s) for s in sets], "records": records, "slots": slots, "repeats": args.repeats,
           "slots_per_s_in_kernels": round(slots / (kernels * 1e-3)) if kernels > 0 else None,
           "slots_per_s_whole_pass": round(slots / min(times["pass_s"]))}
    out.update({k: spread(v) for k, v in times.items()})
    emit(out, args)


if __name__ == "__main__":
    main()
