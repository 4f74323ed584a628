"""The fuzz corpus of tests/read_fuzz.py on the CPU: the census of what it contains, its independent oracle
against the restatements of sections 7f - 7k on every seed, every rule of the oracle shown to be reached, the rows through a BAM
file and back, and the host walks of cigar.h over every corpus as a stand-alone program under AddressSanitizer and UBSan."""
import dataclasses
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import markdup
from hello_amd.bam import BamFile
from tests import qc_cases, read_fuzz as rf
from tests.bam_writer import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPORA = [(seed, profile) for seed in rf.SEEDS for profile in rf.PROFILES]


def test_census_every_situation_really_occurs():
    got = rf.census([rf.corpus(seed, profile) for seed, profile in CORPORA])
    print(dict(got))
    short = {k: got[k] for k in rf.CENSUS_AT_LEAST_5 if got[k] < 5}
    assert not short, short
    assert min(got["observes_a"], got["observes_b"]) >= 0.2 * got["slots"], (got["observes_a"], got["observes_b"], got["slots"])
    assert all(got[k] >= 10 for k in rf.CENSUS_CAUSES), {k: got[k] for k in rf.CENSUS_CAUSES}
    sizes = [len(rf.corpus(seed, "short")[1]) for seed in rf.SEEDS]
    assert 130 <= min(sizes) and max(sizes) <= 150 and all(10 <= len(rf.corpus(seed, "long")[1]) <= 16 for seed in rf.SEEDS)


def test_every_corpus_is_the_pinned_one():
    """The digest over (reference, rows, records) of all 64 corpora, computed before ``corpus`` gained ``reference_of``: with the
    default every corpus stays byte for byte what sections 7l, 7n and 7p were tested on.  With ``reference_of="short"`` a long
    corpus has the short one's chromosome and records and its own reads' CIGARs."""
    h = hashlib.sha256()
    for seed, profile in CORPORA:
        reference, rows, records = rf.corpus(seed, profile)
        h.update(repr((reference, rows, [(r.start, r.end, r.a, r.b, r.allele_a, r.allele_b) for r in records])).encode())
    assert h.hexdigest() == "8bf628aa5311bb0ae2ea763db4cdaaa28fea93f13f9298a4cc796961ecd0dece"
    for seed in (0, 7):
        short, long_, shared = rf.corpus(seed, "short"), rf.corpus(seed, "long"), rf.corpus(seed, "long", reference_of="short")
        assert shared[0] == short[0] and shared[2] == short[2] and shared[0] != long_[0]
        assert all(not r[3] or len(r[4]) >= 512 for r in shared[1])         # the long profile's reads


def test_alignment_table_is_the_plain_expansion():
    """3H 2S 2M 1I 1P 2D 3N 1= 1X at 10: worked by hand."""
    H, S, M, I, P, D, N, EQ, X = rf.H, rf.S, rf.M, rf.I, rf.P, rf.D, rf.N, rf.EQ, rf.X
    rows = [(1, 0, 10, [(H, 3), (S, 2), (M, 2), (I, 1), (P, 1), (D, 2), (N, 3), (EQ, 1), (X, 1)], "ACGTACG", [30] * 7, 60),
            (2, 0, 4, [], "", [], 60), (3, 0, 7, [(M, 1)], "A", [1], 0)]
    t = rf.alignment_table(rows)
    assert t.read.tolist() == [0] * 16 + [2]
    assert t.opi.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 4, 5, 5, 6, 6, 6, 7, 8, 0]
    assert t.op.tolist() == [H] * 3 + [S] * 2 + [M] * 2 + [I, P, D, D, N, N, N, EQ, X, M]
    assert t.q.tolist() == [-1, -1, -1, 0, 1, 2, 3, 4, -1, -1, -1, -1, -1, -1, 5, 6, 0]
    assert t.p.tolist() == [-1, -1, -1, -1, -1, 10, 11, -1, -1, 12, 13, 14, 15, 16, 17, 18, 7]


@pytest.mark.parametrize("profile", rf.PROFILES)
def test_oracle_equals_the_restatements_on_every_seed(profile):
    found = {seed: rf.disagreements(seed, profile) for seed in rf.SEEDS}
    assert not any(found.values()), {seed: names for seed, names in found.items() if names}


@pytest.mark.parametrize("rule", [f.name for f in dataclasses.fields(rf.Rules)])
def test_every_rule_is_reached(rule):
    """The oracle with one rule off differs from the restatement on some seed: the corpus meets the rule, and the comparison above
    would see it broken.  The score's saturation is beyond any read of the grammar and has a read set of its own."""
    off = rf.Rules(**{rule: False})
    if rule == "score_saturated":
        reference, rows = rf.saturating()
        want = markdup.duplicates_of(qc_cases.read_set(rows))[1]
        kept, dropped = rf.Oracle(reference, rows).duplicates(), rf.Oracle(reference, rows, off).duplicates()
        assert want["score"].tolist() == [markdup.MAX_SCORE, 300, 410] and want["duplicate"].tolist() == [0, 1, 1]
        assert all(np.array_equal(kept[k], want[k]) for k in ("e", "score", "kind", "duplicate")) and kept["counts"] == want["counts"]
        assert dropped["score"].tolist() == [255 * len(rows[0][4]), 300, 410] and dropped["score"][0] > markdup.MAX_SCORE
        return
    assert any(rf.disagreements(seed, profile, off) for seed, profile in CORPORA)


@pytest.mark.parametrize("profile", rf.PROFILES)
def test_rows_through_a_bam_and_back(profile, tmp_path):
    for seed in rf.SEEDS:
        reference, rows, _ = rf.corpus(seed, profile)
        want = qc_cases.read_set(rf.bam_rows(rows))
        path = str(tmp_path / ("%s%d.bam" % (profile, seed)))
        write_bam(path, [("chrF", rf.LENGTH)], rf.bam_reads(rows), index=True, block_bytes=997)
        with BamFile(path) as handle:
            got = handle.fetch("chrF", 0, rf.LENGTH)
        assert got.n_reads == len(rows)
        for name in ("bases", "quals", "read_offsets", "cigars", "cigar_offsets", "ref_starts", "mapq", "flags"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (seed, name)
        assert got.name_hash.tolist() == [rf.fnv1a("n%d" % row[0]) for row in rows]
        unmapped = (want.flags & 4) != 0                                  # bam_endpos: an unmapped read ends one behind its start
        assert np.array_equal(got.ref_ends, np.where(unmapped, want.ref_starts + 1, want.ref_ends)), seed


def dump(path, reads):
    with open(path, "wb") as fh:
        fh.write(np.array([reads.n_reads, reads.bases.shape[0], reads.cigars.shape[0]], np.int64).tobytes())
        for a, dtype in ((reads.read_offsets, np.int64), (reads.cigar_offsets, np.int64), (reads.ref_starts, np.int64), (reads.ref_ends, np.int64),
                         (reads.cigars, np.uint32), (reads.flags, np.uint16), (reads.mapq, np.uint8), (reads.bases, np.uint8), (reads.quals, np.uint8)):
            fh.write(np.ascontiguousarray(a, dtype).tobytes())
    return path


def test_host_walks_over_every_corpus_under_sanitizers(tmp_path):
    """strict_walk (kStrictPlain), counted_walk, markdup_walk and qc_walk accept every corpus and classify and measure every read
    as the alignment table does.  The strict walk checks the bases against the BAM's codes, which have no case: it gets the
    upper-cased rows; the other walks do not read the bases."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "walk_corpus")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "walk_corpus.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = []
    for seed, profile in CORPORA:
        rows = rf.corpus(seed, profile)[1]
        files.append(dump(str(tmp_path / ("%s%d.bin" % (profile, seed))), qc_cases.read_set([r[:4] + (r[4].upper(),) + r[5:] for r in rows])))
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.endswith("walk_corpus: ok\n"), (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    parts = run.stdout.split("corpus ")[1:]
    assert len(parts) == len(CORPORA)
    for (seed, profile), part in zip(CORPORA, parts):
        reference, rows, _ = rf.corpus(seed, profile)
        o = rf.Oracle(reference, rows)
        t = o.t
        got = np.array([[int(x) for x in line.split()] for line in part.splitlines()[1:len(rows) + 1]], np.int64)
        qlen, rlen = np.bincount(t.read[t.q >= 0], minlength=o.n), np.bincount(t.read[t.p >= 0], minlength=o.n)
        usable = o.eligible & (((o.flag & 1) == 0) | ((o.flag & 2) != 0)) & (o.mapq > 0)
        covered = np.isin(t.op, rf.ALIGNED + (rf.D,))
        last = np.full(o.n, -1, np.int64)
        np.maximum.at(last, t.read[covered], t.p[covered])
        want = np.stack([np.arange(o.n), o.counted, np.where(o.counted, qlen, -1), np.where(o.counted, rlen, -1), o.eligible,
                         1 + 2 * o.measured + 4 * o.counted, np.where(usable, last, -1)], axis=1)
        assert np.array_equal(got, want), (seed, profile, np.flatnonzero((got != want).any(axis=1))[:5])
        span = int(part.split()[4])
        assert span == int(np.max(np.where(usable, np.maximum(rlen, 1), 0)))
