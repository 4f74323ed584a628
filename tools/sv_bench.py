"""Benchmark of the large deletions and insertions (hello_sv_*) on two synthetic loads: about 200 k reads of
150 bases, and about 20 k reads of 15 kb with several hundred CIGAR operations each.  Per load: the cover, reads and finish kernels'
ms (HIP events, ``hello_sv_stats``), the wall ms of ``hello_sv_add`` and of ``hello_sv_finish``, and the host's own validating walk
of the same reads -- the wall ms of a ``hello_sv_add`` on a handle made for a device that does not exist, which runs the span check,
``sv_walk`` and the kernels' lists and is refused where it opens the device.

    python tools/sv_bench.py [--load short|long|both|split|pairs|pairs_older] [--warmup 2] [--repeats 7] [--profile FILE] [--tree DIR]

``--load split`` is the long load with the 300D of one read in four carried as a split alignment instead: the
primary ends where the deletion begins and the SA tag names the rest of the read.  It reports the split kernel's ms and the wall ms
of ``hello_sv_add_split`` beside the host's walk of the same reads, and, on the long load itself (no read has a tag), the wall ms of
``hello_sv_add`` beside ``hello_sv_add_split`` with empty tags.

``--load pairs`` is the short load with every read made one of a forward-reverse pair of inner distance 150 to
250 and one pair in fifty discordant (its mate 2 000 bases on): the pairs kernel's ms and the wall ms of ``hello_sv_add_pairs``, beside
the wall ms of ``hello_sv_add_split`` and ``hello_sv_add`` on the same reads (no read has a tag) and the host's walk.
``--load pairs_older`` runs those two older adds alone on the same reads and calls nothing newer than section 7q, so with ``--tree
DIR`` (a checkout of another commit with its library built; default: this tree) it measures them there: the line's ``tree`` says
which.

--warmup untimed runs, then --repeats timed ones; prints one JSON line per load with the minimum, the median and the maximum of each
time and, with --profile, appends it to FILE."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT      # before hello_amd is imported
sys.path.insert(0, TREE)

from hello_amd import sv  # noqa: E402
from hello_amd.bam import Reads, Splits  # noqa: E402
try:
    from hello_amd.bam import Mates  # noqa: E402
except ImportError:                                       # --tree of a commit before section 7s: --load pairs_older needs none
    Mates = None

M, I, D = 0, 1, 2


def spread(values):
    v = np.asarray(values, float)
    return {"min": round(float(v.min()), 4), "median": round(float(np.median(v)), 4), "max": round(float(v.max()), 4)}


def synthesize(load: str, seed: int = 1):
    """-> (reference uint8, Reads, the mean operations per read)."""
    rng = np.random.default_rng(seed)
    if load == "short":                                  # 30x over 1 Mb; one read in fifty has a deletion of 60 bases: 45M 60D 105M
        length, n_reads, read_len = 1_000_000, 200_000, 150
        starts = np.sort(rng.integers(0, length - 300, size=n_reads))
        with_event = rng.random(n_reads) < 0.02
        plain, event, before, grid = [(M, 150)], [(M, 45), (D, 60), (M, 105)], 45, 2000
    else:                                                # 30x over 10 Mb; 250 times 29M 1I 29M 1D, and in one read of four a 300D
        length, n_reads, read_len = 10_000_000, 20_000, 15_000
        starts = np.sort(rng.integers(0, length - 16_000, size=n_reads))
        with_event = rng.random(n_reads) < 0.25
        unit = [(M, 29), (I, 1), (M, 29), (D, 1)]
        plain, event, before, grid = unit * 250 + [(M, 250)], unit * 125 + [(D, 300)] + unit * 125 + [(M, 250)], 125 * 59, 50_000
        if load == "split":                              # the read leaves the reference where the deletion begins; the tag has the rest
            event = unit * 125 + [(4, read_len - 125 * 59)]
    # the events lie on a grid, so that clusters form
    starts[with_event] = np.maximum((starts[with_event] + before) // grid * grid, grid) - before
    order = np.argsort(starts, kind="stable")
    starts, with_event = starts[order], with_event[order]
    reference = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length)
    packed = [np.array([n << 4 | op for op, n in ops], np.uint32) for ops in (plain, event)]
    which = with_event.astype(np.int64)
    cigars = np.concatenate([packed[k] for k in which])
    cigar_offsets = np.concatenate([[0], np.cumsum(np.array([len(plain), len(event)])[which])]).astype(np.int64)
    on_ref = np.array([sum(n for op, n in ops if op in (M, D)) for ops in (plain, event)], np.int64)[which]
    on_read = np.array([sum(n for op, n in ops if op != D) for ops in (plain, event)], np.int64)[which]
    assert int(on_read.min()) == int(on_read.max()) == read_len
    n_bases = int(on_read.sum())
    reads = Reads(bases=rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n_bases), quals=np.full(n_bases, 30, np.uint8),
                  read_offsets=np.concatenate([[0], np.cumsum(on_read)]).astype(np.int64), cigars=cigars, cigar_offsets=cigar_offsets,
                  ref_starts=starts.astype(np.int64), ref_ends=(starts + on_ref).astype(np.int64), mapq=np.full(n_reads, 60, np.uint8),
                  flags=(rng.integers(0, 2, size=n_reads) * 0x10).astype(np.uint16), name_hash=np.arange(n_reads, dtype=np.uint64),
                  strand=np.zeros(n_reads, np.uint8), hp=rng.integers(0, 3, size=n_reads).astype(np.uint8))
    if load == "split":
        tags = [b"chr1,%d,%s,%dS%dM,60,7;" % (s + 125 * 60 + 300 + 1, b"-" if f else b"+", 125 * 59, read_len - 125 * 59) if e else b""
                for s, e, f in zip(starts, with_event, reads.flags)]                 # the other segment lies on the primary's strand
        splits = Splits(np.frombuffer(b"".join(tags), np.uint8).copy(), np.concatenate([[0], np.cumsum([len(t) for t in tags])]).astype(np.int64))
        return reference, reads, float(np.diff(cigar_offsets).mean()), splits
    return reference, reads, float(np.diff(cigar_offsets).mean())


def host_walk_ms(reference, reads, splits=None) -> float:
    """The wall ms of an add that is refused where it opens the device: the span check, sv_walk and the kernels' lists."""
    with sv.Caller(reference, device=1 << 20) as caller:
        if splits is not None:
            caller.set_contigs(["chr1", "chr2"], 0)
        t0 = time.perf_counter()
        try:
            caller.add(reads, 0, reference.shape[0], splits=splits)
        except RuntimeError as refused:
            if "device" not in str(refused):
                raise
        else:
            raise RuntimeError("the add on a device that does not exist was not refused")
        return (time.perf_counter() - t0) * 1e3


def run_split(warmup: int, repeats: int) -> dict:
    reference, reads, ops, splits = synthesize("split")
    _, untagged, _ = synthesize("long")
    empty = Splits(np.zeros(0, np.uint8), np.zeros(untagged.n_reads + 1, np.int64))
    names = ("split_ms", "reads_ms", "cover_ms", "add_split_wall_ms", "host_walk_ms", "no_sa_add_wall_ms", "no_sa_add_split_wall_ms")
    times = {k: [] for k in names}
    counts = {}
    for n in range(warmup + repeats):
        with sv.Caller(reference) as caller:
            caller.set_contigs(["chr1", "chr2"], 0)
            t0 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0], splits=splits)
            t1 = time.perf_counter()
            caller.finish()
            stats = caller.stats()
        walk = host_walk_ms(reference, reads, splits)
        with sv.Caller(reference) as caller:
            t2 = time.perf_counter()
            caller.add(untagged, 0, reference.shape[0])
            t3 = time.perf_counter()
        with sv.Caller(reference) as caller:
            caller.set_contigs(["chr1", "chr2"], 0)
            t4 = time.perf_counter()
            caller.add(untagged, 0, reference.shape[0], splits=empty)
            t5 = time.perf_counter()
        if n < warmup:
            continue
        for k in names[:3]:
            times[k].append(stats[k])
        for k, v in zip(names[3:], ((t1 - t0) * 1e3, walk, (t3 - t2) * 1e3, (t5 - t4) * 1e3)):
            times[k].append(v)
        counts = {k: int(stats[k]) for k in sv.COUNT_NAMES + sv.SPLIT_COUNT_NAMES}
    return dict(load="split", reads=reads.n_reads, bases=int(reads.bases.shape[0]), sa_bytes=int(splits.bytes.shape[0]),
                operations_per_read=round(ops, 1), reference_bases=int(reference.shape[0]), warmup=warmup, repeats=repeats, **counts,
                **{k: spread(v) for k, v in times.items()})


def paired(reads: Reads, length: int, seed: int = 2):
    """The short load's reads as left records of forward-reverse pairs (no mate record: a right record only counts), one in fifty
    without flag 0x2 and with its mate 2 000 bases on -> (Reads, Splits without a tag, Mates)."""
    rng = np.random.default_rng(seed)
    n = reads.n_reads
    discordant = rng.random(n) < 0.02
    inner = np.where(discordant, 2000, rng.integers(150, 251, size=n))
    mates = Mates(np.zeros(n, np.int32), np.minimum(reads.ref_ends + inner, length).astype(np.int64), np.zeros(n, np.int32)) if Mates else None
    flags = np.where(discordant, 0x1 | 0x20 | 0x40, 0x1 | 0x2 | 0x20 | 0x40).astype(np.uint16)
    return dataclasses.replace(reads, flags=flags), Splits(np.zeros(0, np.uint8), np.zeros(n + 1, np.int64)), mates


def run_pairs_older(warmup: int, repeats: int) -> dict:
    reference, reads, ops = synthesize("short")
    reads, empty, _ = paired(reads, reference.shape[0])
    names = ("reads_ms", "cover_ms", "add_split_wall_ms", "add_wall_ms")
    times = {k: [] for k in names}
    counts = {}
    for n in range(warmup + repeats):
        with sv.Caller(reference) as caller:
            caller.set_contigs(["chr1", "chr2"], 0)
            t0 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0], splits=empty)
            t1 = time.perf_counter()
            stats = caller.stats()
        with sv.Caller(reference) as caller:
            t2 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0])
            t3 = time.perf_counter()
        if n < warmup:
            continue
        for k, v in zip(names, (stats["reads_ms"], stats["cover_ms"], (t1 - t0) * 1e3, (t3 - t2) * 1e3)):
            times[k].append(v)
        counts = {k: int(stats[k]) for k in ("counting", "signatures")}
    return dict(load="pairs_older", tree="this" if TREE == ROOT else os.path.basename(TREE), reads=reads.n_reads, warmup=warmup,
                repeats=repeats, **counts, **{k: spread(v) for k, v in times.items()})


def run_pairs(warmup: int, repeats: int) -> dict:
    reference, reads, ops = synthesize("short")
    reads, empty, mates = paired(reads, reference.shape[0])
    library = (200, 100, 300)
    names = ("pairs_ms", "reads_ms", "cover_ms", "finish_ms", "add_pairs_wall_ms", "add_split_wall_ms", "add_wall_ms", "host_walk_ms")
    times = {k: [] for k in names}
    counts = {}
    for n in range(warmup + repeats):
        with sv.Caller(reference) as caller:
            caller.set_contigs(["chr1", "chr2"], 0)
            caller.set_library(*library)
            t0 = time.perf_counter()
            caller.add(reads, empty, mates, 0, reference.shape[0])
            t1 = time.perf_counter()
            caller.finish()
            stats = caller.stats()
        with sv.Caller(reference) as caller:
            caller.set_contigs(["chr1", "chr2"], 0)
            t2 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0], splits=empty)
            t3 = time.perf_counter()
        with sv.Caller(reference) as caller:
            t4 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0])
            t5 = time.perf_counter()
        walk = host_walk_ms(reference, reads)
        if n < warmup:
            continue
        for k in names[:4]:
            times[k].append(stats[k])
        for k, v in zip(names[4:], ((t1 - t0) * 1e3, (t3 - t2) * 1e3, (t5 - t4) * 1e3, walk)):
            times[k].append(v)
        counts = {k: int(stats[k]) for k in sv.COUNT_NAMES + sv.PAIR_COUNT_NAMES}
    return dict(load="pairs", reads=reads.n_reads, bases=int(reads.bases.shape[0]), reference_bases=int(reference.shape[0]), library=library,
                warmup=warmup, repeats=repeats, **counts, **{k: spread(v) for k, v in times.items()})


def run(load: str, warmup: int, repeats: int) -> dict:
    if load == "split":
        return run_split(warmup, repeats)
    if load == "pairs":
        return run_pairs(warmup, repeats)
    if load == "pairs_older":
        return run_pairs_older(warmup, repeats)
    reference, reads, ops = synthesize(load)
    times = {k: [] for k in ("cover_ms", "reads_ms", "finish_ms", "add_wall_ms", "finish_wall_ms", "host_walk_ms")}
    counts = {}
    for n in range(warmup + repeats):
        with sv.Caller(reference) as caller:
            t0 = time.perf_counter()
            caller.add(reads, 0, reference.shape[0])
            t1 = time.perf_counter()
            caller.finish()
            t2 = time.perf_counter()
            stats = caller.stats()
        walk = host_walk_ms(reference, reads)
        if n < warmup:
            continue
        for k in ("cover_ms", "reads_ms", "finish_ms"):
            times[k].append(stats[k])
        times["add_wall_ms"].append((t1 - t0) * 1e3)
        times["finish_wall_ms"].append((t2 - t1) * 1e3)
        times["host_walk_ms"].append(walk)
        counts = {k: int(stats[k]) for k in sv.COUNT_NAMES}
    return dict(load=load, reads=reads.n_reads, bases=int(reads.bases.shape[0]), operations_per_read=round(ops, 1),
                reference_bases=int(reference.shape[0]), warmup=warmup, repeats=repeats, **counts, **{k: spread(v) for k, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--load", choices=["short", "long", "both", "split", "pairs", "pairs_older"], default="both")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--profile", help="append every JSON line to this file")
    ap.add_argument("--tree", help="the checkout whose hello_amd and library are measured (default: this one); for --load pairs_older")
    args = ap.parse_args()
    for load in (("short", "long") if args.load == "both" else (args.load,)):
        line = json.dumps(run(load, args.warmup, args.repeats))
        print(line, flush=True)
        if args.profile:
            with open(args.profile, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
