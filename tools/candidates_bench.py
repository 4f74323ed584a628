"""Candidate stage benchmark on the synthetic chromosome of tools/hotspot_bench.py: hotspot positions -> candidate sites timed
end to end (BAM decode included) and split into BAM decode, the three kernels (HIP events), the host gather and the rest of
the call (planning, transfers), plus the CPU restatement (tests/candidate_reference.py) on a slice for context.

    python tools/candidates_bench.py [--length 5000000] [--coverage 30] [--read-length 150] [--slice 20000] [--repeats 5] [--pacbio]
    python tools/candidates_bench.py --hybrid [--pacbio-coverage 25] [--pacbio-read-length 3000] [--hybrid_hotspot] ...

--pacbio: the reads are treated as PacBio reads (give a --read-length of several thousand): PacBio hotspots, the read cap of 100
per 100 bp, strict clipping -- the two clip kernels are timed with the other stages (clip_kernel_ms).

--hybrid: an Illumina BAM (--coverage, --read-length) and a PacBio BAM (--pacbio-coverage, --pacbio-read-length) of the same donor
through hello_candidates_find_hybrid: the same stage times plus the reassembly phase (reassembly_ms) and its counts, against
tests/hybrid_reference.py on the slice.

--resident [--profile FILE]: the resident route (HELLO_CANDIDATES_RESIDENT) beside the host route.  For the Illumina, the --pacbio
and the --hybrid input, each in a child process of its own under `timeout`, stopping at the first that fails: in one process and
on one input the host gather's ms (the statistic of a non-resident call) beside the gather kernel's ms (HIP events on its stream),
both calls' total ms, and the ms of uploading the whole chromosome as every call does.  Then the wall time of
`python -m hello_amd.call --from_bam` with and without --resident on one synthetic chromosome (--call-length), three interleaved
runs each.  Every JSON line is printed and, with --profile, appended to FILE.

One warm-up run, then --repeats timed runs; prints one JSON line with the minimum, the median and the spread of each time."""
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
    ap.add_argument("--hybrid", action="store_true", default=False, help="an Illumina and a PacBio BAM together: the reassembly phase's time too")
    ap.add_argument("--pacbio-coverage", type=float, default=25)
    ap.add_argument("--pacbio-read-length", type=int, default=3000)
    ap.add_argument("--hybrid_hotspot", action="store_true", default=False)
    ap.add_argument("--resident", action="store_true", default=False, help="the resident route beside the host route (see above)")
    ap.add_argument("--resident-step", choices=["illumina", "pacbio", "hybrid", "call"], help="one step of --resident (its child processes)")
    ap.add_argument("--call-length", type=int, default=200_000, help="--resident: the chromosome of the call --from_bam runs")
    ap.add_argument("--step-timeout", type=int, default=420, help="--resident: seconds each child process may take")
    ap.add_argument("--profile", help="--resident: append the JSON lines to this file")
    args = ap.parse_args()
    if args.resident_step:
        return resident_step(args)
    if args.resident:
        return resident(args)
    if args.hybrid:
        return hybrid(args)
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


def pacbio_noise(read, rng, rate=0.01):
    """`read` with PacBio-like errors inside its M operations, as tests/hotspot_synth._pacbio_noise draws them: a base is dropped
    (a 1-base deletion) with probability `rate`, a random base is inserted before it with the same probability."""
    seq, qual, cigar, rd = [], [], [], 0

    def push(op, n):
        if n > 0:
            if cigar and cigar[-1][0] == op:
                cigar[-1] = (op, cigar[-1][1] + n)
            else:
                cigar.append((op, n))
    for op, n in read.cigar:
        if op != 0:
            if op in (1, 4):
                seq.append(read.seq[rd:rd + n]); qual.append(read.qual[rd:rd + n]); rd += n
            push(op, n)
            continue
        u = rng.random(n)
        events = np.nonzero(u < 2 * rate)[0]
        at = 0
        for e in events:
            e = int(e)
            if e == 0 and not cigar:
                continue                                       # the read keeps its first aligned base
            seq.append(read.seq[rd + at:rd + e]); qual.append(read.qual[rd + at:rd + e]); push(0, e - at)
            if u[e] < rate:
                push(2, 1)
                at = e + 1
            else:
                seq.append("ACGT"[int(rng.integers(0, 4))]); qual.append(read.qual[rd + e:rd + e + 1]); push(1, 1)
                at = e
        seq.append(read.seq[rd + at:rd + n]); qual.append(read.qual[rd + at:rd + n]); push(0, n - at)
        rd += n
    if cigar[-1][0] == 2:                                      # no deletion at the read's end
        cigar.pop()
    return type(read)("p" + read.name, read.pos, cigar, "".join(seq), b"".join(bytes(q) for q in qual), read.flag, read.mapq)


def hybrid(args):
    from hello_amd import hotspots as hs, hybrid as hb
    from hello_amd.bam import BamFile
    from tests import hybrid_reference as hy
    ref, illumina = synthesize(args.length, args.coverage, args.read_length)
    ref1, pacbio = synthesize(args.length, args.pacbio_coverage, args.pacbio_read_length)      # the same seed: the same donor
    assert ref1 == ref
    noise = np.random.default_rng(7)
    pacbio = [pacbio_noise(r, noise) for r in pacbio]           # misaligned single-base indels: what the reassembly reconciles
    names = ("pass1_kernel_ms", "pass2_kernel_ms", "allele_kernel_ms", "clip_kernel_ms", "reassembly_ms", "gather_ms")
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, "i.bam"), os.path.join(d, "p.bam")]
        for path, reads in zip(paths, (illumina, pacbio)):
            write_bam(path, [("chr1", len(ref))], reads, index=True)

        def decode():
            out = []
            for path in paths:
                with BamFile(path) as b:
                    out.append(b.fetch("chr1", 0, len(ref)))
            return out
        positions, _ = hs.find_positions(decode(), ref, [(0, len(ref))], hybrid_hotspot=args.hybrid_hotspot)
        times = {k: [] for k in ("end_to_end_s", "bam_decode_s", "call_s", "call_rest_ms") + names}
        st = {}
        for i in range(args.repeats + 1):
            t0 = time.perf_counter()
            r0, r1 = decode()
            t1 = time.perf_counter()
            shard, st, _ = hb.find_sites(r0, r1, ref, positions, "chr1", hybrid_hotspot=args.hybrid_hotspot)
            t2 = time.perf_counter()
            if i == 0:
                continue
            for k, v in (("end_to_end_s", t2 - t0), ("bam_decode_s", t1 - t0), ("call_s", t2 - t1),
                         ("call_rest_ms", st["total_ms"] - sum(st[k] for k in names))):
                times[k].append(v)
            for k in names:
                times[k].append(st[k])
        a = len(ref) // 2
        sl_pos = [int(p) for p in positions if a <= p < a + args.slice]
        sl0 = [x for x in illumina if x.pos < a + args.slice + 200 and x.ref_end > a - 200]
        sl1 = [x for x in pacbio if x.pos < a + args.slice + 200 and x.ref_end > a - 200]
        t = time.perf_counter()
        want = hy.find_candidates(sl0, sl1, ref, sl_pos, hybrid_hotspot=args.hybrid_hotspot)
        t_cpu = time.perf_counter() - t
    sites = int(st["sites"])
    out = {"hybrid": True, "hybrid_hotspot": bool(args.hybrid_hotspot), "length": args.length, "coverage": args.coverage,
           "pacbio_coverage": args.pacbio_coverage, "reads": [len(illumina), len(pacbio)], "positions": int(len(positions)), "sites": sites,
           "repeats": args.repeats, "sites_per_s_end_to_end": round(sites / min(times["end_to_end_s"])),
           "sites_per_s_without_bam_decode": round(sites / min(times["call_s"])),
           "slice_bp": args.slice, "slice_sites": len(want), "slice_cpu_restatement_s": round(t_cpu, 3),
           "cpu_restatement_sites_per_s": round(len(want) / max(t_cpu, 1e-9), 1)}
    out.update({k: int(st[k]) for k in ("alleles", "reads_gathered", "record_slots", "active_regions", "clusters", "reads_clipped",
                                        "clusters_gate_passed", "clusters_reassembled", "pacbio_reads_eligible", "pacbio_reads_reassigned",
                                        "pacbio_reads_reassigned_by_tie", "illumina_sites")})
    out.update({k: spread(v) for k, v in times.items()})
    print(json.dumps(out))


def resident(args):
    """The steps of --resident, each a child process under its own time limit; the first failure ends the run."""
    common = ["--length", str(args.length), "--coverage", str(args.coverage), "--read-length", str(args.read_length), "--repeats",
              str(args.repeats), "--pacbio-coverage", str(args.pacbio_coverage), "--pacbio-read-length", str(args.pacbio_read_length),
              "--call-length", str(args.call_length)]
    for step in ("illumina", "pacbio", "hybrid", "call"):
        done = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--resident-step",
                               step] + common, capture_output=True, text=True)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-3000:])
            raise SystemExit(f"step {step} ended with status {done.returncode}: nothing further is started")
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if args.profile:
            with open(args.profile, "a") as fh:
                fh.write(line + "\n")


def resident_step(args):
    if args.resident_step == "call":
        return resident_call(args)
    import torch
    from hello_amd import candidates as cd, hotspots as hs, hybrid as hb
    from hello_amd.bam import BamFile
    from hello_amd.resident import GATHER_ARRAYS
    kind = args.resident_step
    ref, reads = synthesize(args.length, args.coverage, args.read_length) if kind != "pacbio" else synthesize(
        args.length, args.pacbio_coverage, args.pacbio_read_length)
    sets = [reads]
    if kind == "hybrid":
        _, pacbio = synthesize(args.length, args.pacbio_coverage, args.pacbio_read_length)
        noise = np.random.default_rng(7)
        sets.append([pacbio_noise(r, noise) for r in pacbio])
    sizes = dict(bases=1, quals=1, read_off=8, cigars=4, cigar_off=8, ref_start=8, mapq=1, orientation=1, hp=1, site_of_read=4)
    stream = torch.cuda.Stream()
    with tempfile.TemporaryDirectory() as d:
        decoded = []
        for i, rs in enumerate(sets):
            path = os.path.join(d, f"{i}.bam")
            write_bam(path, [("chr1", len(ref))], rs, index=True)
            with BamFile(path) as b:
                decoded.append(b.fetch("chr1", 0, len(ref)))
    positions, _ = hs.find_positions(decoded, ref, [(0, len(ref))], pacbio=kind == "pacbio")

    def find(resident):
        if kind == "hybrid":
            return hb.find_sites(decoded[0], decoded[1], ref, positions, "chr1", resident=resident)
        return cd.find_sites(decoded[0], ref, positions, "chr1", options=hs.HOTSPOTS_PACBIO if kind == "pacbio" else 0, resident=resident)
    times = {k: [] for k in ("host_gather_ms", "host_route_call_ms", "gather_kernel_ms", "resident_call_ms", "reference_upload_ms")}
    chromosome = torch.from_numpy(np.frombuffer(ref.encode("latin-1"), np.uint8).copy())
    on_device = torch.empty(len(ref), dtype=torch.uint8, device="cuda")
    out = {}
    for i in range(args.repeats + 1):
        _, st, _ = find(False)
        shard, rst, _ = find(True)
        with shard:
            techs = (0, 1) if kind == "hybrid" else (0,)
            counts = {t: shard.featurizer_counts(t) for t in techs}
            buffers = {}
            for t in techs:
                n, nb, nc = counts[t]
                want = dict(bases=nb, quals=nb, read_off=n + 1, cigars=nc, cigar_off=n + 1, ref_start=n, mapq=n, orientation=n, hp=n,
                            site_of_read=n)
                buffers[t] = {k: torch.empty(want[k] * sizes[k] + 16, dtype=torch.uint8, device="cuda") for k in GATHER_ARRAYS}
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for t in techs:
                shard.gather(t, {k: b.data_ptr() for k, b in buffers[t].items()}, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            kernel_ms = e0.elapsed_time(e1)
            out = {"sites": shard.n_sites, "featurizer_reads": [counts[t][0] for t in techs], "gathered_bytes": [2 * counts[t][1] + 4 * counts[t][2] for t in techs]}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_device.copy_(chromosome)
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        if i == 0:
            continue
        for k, v in (("host_gather_ms", st["gather_ms"]), ("host_route_call_ms", st["total_ms"]), ("gather_kernel_ms", kernel_ms),
                     ("resident_call_ms", rst["total_ms"]), ("reference_upload_ms", upload_ms)):
            times[k].append(v)
    out.update({"resident": kind, "length": args.length, "reads": [len(r) for r in sets], "positions": int(len(positions)), "repeats": args.repeats})
    out.update({k: spread(v) for k, v in times.items()})
    print(json.dumps(out))


def resident_call(args):
    """Wall seconds of python -m hello_amd.call --from_bam on one synthetic chromosome through shard files and with --resident,
    three runs each, interleaved; every run a child process under its own time limit."""
    from hello_amd import loader, netspec as ns, weights
    ref, reads = synthesize(args.call_length, args.coverage, args.read_length)
    times = {"shard_files_s": [], "resident_s": []}
    with tempfile.TemporaryDirectory() as d:
        bam, fa, model = os.path.join(d, "x.bam"), os.path.join(d, "g.fa"), os.path.join(d, "model.hello.npz")
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        with open(fa, "w") as fh:
            fh.write(">chr1\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=17))
        vcfs = {}
        for i in range(3):
            for key, extra in (("shard_files_s", []), ("resident_s", ["--resident"])):
                work = os.path.join(d, f"{key}{i}")
                t0 = time.perf_counter()
                done = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, "-m", "hello_amd.call", "--ibam", bam,
                                       "--ref", fa, "--workdir", work, "--network", model, "--from_bam"] + extra, cwd=ROOT,
                                      capture_output=True, text=True)
                times[key].append(time.perf_counter() - t0)
                if done.returncode != 0:
                    sys.stderr.write(done.stderr[-3000:])
                    raise SystemExit(f"call {key} ended with status {done.returncode}")
                vcfs[key] = open(os.path.join(work, "results.output.vcf"), "rb").read()
                shard_bytes = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(work) for f in fs if f.endswith(".hshard"))
                if key == "shard_files_s":
                    files_bytes = shard_bytes
                else:
                    assert shard_bytes == 0
        assert vcfs["shard_files_s"] == vcfs["resident_s"]
    out = {"resident": "call --from_bam", "length": args.call_length, "reads": len(reads), "hshard_bytes_of_the_file_route": files_bytes, "records": sum(1 for line in vcfs["resident_s"].splitlines() if not line.startswith(b"#"))}
    out.update({k: spread(v) for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
