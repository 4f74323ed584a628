"""Hotspot stage benchmark: a synthetic chromosome written to a temporary BAM (+ .bai), then BAM decode, the GPU kernel and the
end-to-end call timed, and the CPU restatement (tests/hotspot_reference.py) timed on a slice for the ratio.

    python tools/hotspot_bench.py [--length 5000000] [--coverage 30] [--read-length 150] [--slice 20000]

Prints one JSON line: bam_decode_s, kernel_ms (HIP events), end_to_end_s, aligned bases per second, and the CPU
restatement's seconds on the slice against the GPU path's on the same slice (positions checked equal)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import hotspot_reference as hr  # noqa: E402
from tests.bam_writer import Read, write_bam  # noqa: E402

BASES = np.frombuffer(b"ACGT", np.uint8)


def synthesize(length, coverage, read_len, seed=1, snv_rate=0.01, indel_rate=0.001, error_rate=0.002):
    """Reads of a donor with SNVs and short indels, vectorised where it matters (an indel touches few reads)."""
    rng = np.random.default_rng(seed)
    ref = BASES[rng.integers(0, 4, size=length)]
    donor = ref.copy()
    snv = rng.random(length) < snv_rate
    donor[snv] = BASES[(np.searchsorted(BASES, donor[snv]) + rng.integers(1, 4, size=int(snv.sum()))) % 4]
    ev_pos = np.sort(rng.choice(np.arange(200, length - 200), size=int(length * indel_rate), replace=False))
    ev_del = rng.random(ev_pos.size) < 0.5
    ev_len = rng.integers(1, 7, size=ev_pos.size)
    n_reads = int(coverage * length / read_len)
    starts = np.sort(rng.integers(0, length - 2 * read_len, size=n_reads))
    quals = rng.integers(20, 41, size=(n_reads, read_len)).astype(np.uint8)
    reads = []
    for i, s in enumerate(starts):
        s = int(s)
        lo, hi = np.searchsorted(ev_pos, s + 1), np.searchsorted(ev_pos, s + read_len - 10)
        if lo == hi:
            seq, cigar = donor[s:s + read_len].copy(), [(0, read_len)]
        else:                                                   # the first indel in the read only
            p, d, n = int(ev_pos[lo]), bool(ev_del[lo]), int(ev_len[lo])
            m = p - s
            if d:
                seq = np.concatenate([donor[s:p], donor[p + n:p + n + read_len - m]])
                cigar = [(0, m), (2, n), (0, read_len - m)]
            else:
                ins = BASES[rng.integers(0, 4, size=n)]
                seq = np.concatenate([donor[s:p], ins, donor[p:p + read_len - m - n]])
                cigar = [(0, m), (1, n), (0, read_len - m - n)]
        err = rng.random(read_len) < error_rate
        seq[err] = BASES[rng.integers(0, 4, size=int(err.sum()))]
        reads.append(Read(f"r{i}", s, cigar, seq.tobytes().decode(), quals[i].tobytes(), 16 * (i & 1), 60))
    return ref.tobytes().decode(), reads


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=float, default=30)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--slice", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from hello_amd import hotspots as hs
    from hello_amd.bam import BamFile

    t = time.perf_counter()
    ref, reads = synthesize(args.length, args.coverage, args.read_length)
    t_syn = time.perf_counter() - t
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "x.bam")
        t = time.perf_counter()
        write_bam(bam, [("chr1", len(ref))], reads, index=True)
        t_write = time.perf_counter() - t
        bases = sum(len(r.seq) for r in reads)
        decode, kernel, e2e, stats = [], [], [], {}
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            with BamFile(bam) as b:
                r = b.fetch("chr1", 0, len(ref))
            t1 = time.perf_counter()
            pos, stats = hs.find_positions([r], ref, [(0, len(ref))])
            t2 = time.perf_counter()
            decode.append(t1 - t0)
            kernel.append(stats["kernel_ms"])
            e2e.append(t2 - t0)
        # the CPU restatement on a slice, and the GPU path on the same slice
        a = len(ref) // 2
        sl = [x for x in reads if x.pos < a + args.slice and x.ref_end > a]
        t = time.perf_counter()
        want = hr.find_hotspots([sl], ref, a, a + args.slice)
        t_cpu = time.perf_counter() - t
        t = time.perf_counter()
        got = hs.find_hotspots(bam, None, "chr1", a, a + args.slice, reference=ref)
        t_gpu = time.perf_counter() - t
        assert got.tolist() == want, "GPU and restatement disagree on the slice"
    best = int(np.argmin(e2e))
    out = {
        "length": args.length, "coverage": args.coverage, "read_length": args.read_length, "reads": len(reads),
        "aligned_bases": bases, "positions": int(len(pos)), "synthesis_s": round(t_syn, 2), "bam_write_s": round(t_write, 2),
        "bam_decode_s": round(min(decode), 4), "kernel_ms": round(min(kernel), 3), "end_to_end_s": round(min(e2e), 4),
        "plan_ms": round(stats["plan_ms"], 2), "call_total_ms": round(stats["total_ms"], 2),
        "aligned_bases_per_s_end_to_end": round(bases / e2e[best]), "aligned_bases_per_s_kernel": round(bases / (min(kernel) / 1e3)),
        "tiles": int(stats["tiles"]), "chunks": int(stats["chunks"]),
        "slice_bp": args.slice, "slice_cpu_restatement_s": round(t_cpu, 3), "slice_gpu_path_s": round(t_gpu, 3),
        "slice_ratio_cpu_over_gpu": round(t_cpu / t_gpu, 1), "slice_positions": len(want),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
