"""Read-backed phasing on the GPU (hello_phase_*, hello_amd/csrc/phase.hip): every slot, link, set, flip, hp and ps equals the
restatement of hello_amd/phase.py exactly -- on the tables worked by hand and on a 6 kb chromosome of about 170 phasable records
with a stretch of one record every 8 bp (tests/phase_cases.py); ``python -m hello_amd.call --phase`` writes the file the
restatement writes and leaves results.output.vcf and results.output.g.vcf as they were.  The seed was chosen with the restatement
on the CPU so that the conditions asserted in ``chromosome`` hold."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

from hello_amd import phase
from hello_amd.bam import BamFile
from tests import phase_cases as pc
from tests.bam_writer import write_bam
from tests.gvcf_cases import reads_of_bam_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1
MODEL_SEED = 1
PER_READ = ("slots", "slot_offsets", "first", "hp", "ps")
PER_RECORD = ("links", "set", "flip")


def per_read(slots, offsets):
    return [slots[int(offsets[i]):int(offsets[i + 1])].tolist() for i in range(len(offsets) - 1)]


# ---- (1) the hand tables through the kernels --------------------------------------------------------------------------------
def test_hand_table_observations():
    for case in pc.OBSERVE_TABLE:
        got, stats = phase.find_observations([pc.reads_of(case.reads)], case.records)
        assert got["slots"].dtype == np.int8 and per_read(got["slots"], got["slot_offsets"]) == case.slots, case.name
        assert stats["slots"] == sum(len(s) for s in case.slots) and stats["records"] == len(case.records), case.name


def test_hand_table_links_and_haplotags():
    got, _ = phase.find_observations([pc.reads_of(pc.LINK_READS)], pc.LINK_RECORDS, window=pc.LINK_WINDOW)
    assert per_read(got["slots"], got["slot_offsets"]) == pc.LINK_SLOTS
    assert got["links"].dtype == np.int32 and got["links"].tolist() == pc.LINKS
    wide, _ = phase.find_observations([pc.reads_of(pc.LINK_READS)], pc.LINK_RECORDS, window=3)
    assert wide["links"][:, :2].tolist() == pc.LINKS and wide["links"][3, 2].tolist() == [0, 1] and not wide["links"][:3, 2].any()
    # the reads of tests/test_phase.py::test_write_phased_vcf_against_a_file_written_by_hand: three of either haplotype and one that
    # sees the unlinked record only; record 13 is flipped
    from tests.test_phase import INPUT
    records = [r for r in (phase.phasable(line.encode()) for line in INPUT if line.startswith("chrB")) if r]
    hap1, hap2 = "AAAAGAAAAAAACAAAAAAA", "AAAATAAACAAAGAAAAAAA"
    reads = [(0, [(pc.M, 20)], hap1, [30] * 20, 0, 60)] * 3 + [(0, [(pc.M, 20)], hap2, [30] * 20, 0, 60)] * 3 \
        + [(25, [(pc.M, 10)], "AAAATAAAAA", [30] * 10, 0, 60), (0, [(pc.M, 20)], hap1, [30] * 20, 0x400, 60)]
    details = {}
    hp, ps = phase.find_haplotags([pc.reads_of(reads)], records, details=details)
    assert details["set"].tolist() == [0, 0, 0, 3] and details["flip"].tolist() == [0, 0, 1, 0]
    assert hp.dtype == np.uint8 and ps.dtype == np.int64
    assert hp.tolist() == [1, 1, 1, 2, 2, 2, 0, 0] and ps.tolist() == [5] * 6 + [0, 0]


def test_refusals_before_the_launch():
    beyond = pc.reads_of([(0, [(pc.M, 9)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(RuntimeError, match="consumes 9 bases, it has 8"):
        phase.find_observations([beyond], [pc.G_T])
    fine = pc.reads_of([(0, [(pc.M, 8)], "ACGTGCAT", [30] * 8, 0, 60)])
    with pytest.raises(RuntimeError, match="not sorted"):
        phase.find_observations([fine], [pc.snp(6, "A", "C"), pc.G_T])
    with pytest.raises(RuntimeError, match="window"):
        phase.find_observations([fine], [pc.G_T], window=33)
    got, stats = phase.find_observations([fine], [])                                             # no record: no slot, nothing launched
    assert got["slots"].shape == (0,) and got["slot_offsets"].tolist() == [0, 0] and got["links"].shape == (0, 8, 2)
    assert stats["observe_ms"] == 0 and phase.find_haplotags([fine], [])[0].tolist() == [0]


# ---- (2) the 6 kb chromosome --------------------------------------------------------------------------------------------------
_made: dict = {}


def restatement(sets, records):
    slots, offsets, first = phase.slots_of(sets, records)
    links = phase.links_of(slots, offsets, first, len(records), pc.WINDOW)
    chained = phase.chain(links, pc.WINDOW, 2)
    hp, ps = phase.haplotags_of(slots, offsets, first, chained[0], chained[1], [r.pos for r in records])
    return dict(slots=slots, slot_offsets=offsets, first=first, links=links, set=chained[0], flip=chained[1], hp=hp, ps=ps)


def chromosome():
    """The input and its restatement for two sources, computed once, with the conditions that make the comparison worth something."""
    if not _made:
        reference, lines, short, long = pc.synthetic(SEED)
        records = [r for r in map(phase.phasable, lines) if r]
        sets = [reads_of_bam_records(short), reads_of_bam_records(long)]
        want = restatement(sets, records)
        rd = phase._one(sets)
        sizes = collections.Counter(want["set"].tolist())
        assert 150 < len(records) < len(lines) and any(r.a == 1 and r.b == 2 for r in records)
        assert any(len(r.allele_a) != len(r.allele_b) for r in records)                          # indel records
        assert max(sizes.values()) >= 5 and want["flip"].any()                                   # a set of 5 or more, a flip
        assert sum(1 for n in sizes.values() if n == 1) >= 1                                     # an unphased heterozygous record
        why = collections.Counter()
        for r in range(rd.n_reads):
            for j in range(int(want["slot_offsets"][r + 1] - want["slot_offsets"][r])):
                why[phase.observe_why(rd, r, records[int(want["first"][r]) + j])[1]] += 1
        assert all(why[cause] >= 1 for cause in ("neither", "quality", "end", "N")), why         # a none of every cause
        assert why[""] > 1000 and set(want["hp"].tolist()) == {0, 1, 2}
        assert want["links"][:, pc.WINDOW - 1].any()                                              # links at k = W
        per = np.diff(want["slot_offsets"])
        assert per.max() > 64 and (per[phase.counted_mask(rd)] == 0).any()                       # more than one round; no candidate
        assert max(len(r.cigar) for r in long) >= 300 and any(r.flag & 0x400 for r in short)
        gaps = np.diff([r.start for r in records])
        assert gaps.max() > 150 and (gaps == 8).sum() > 64
        _made.update(reference=reference, lines=lines, short=short, long=long, records=records, sets=sets, want=want)
    return _made


def same(got, want, names=PER_READ + PER_RECORD):
    for name in names:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


def observed(sets, records):
    details = {}
    hp, ps = phase.find_haplotags(sets, records, window=pc.WINDOW, details=details)
    return dict(details, hp=hp, ps=ps)


def test_two_sources_equal_the_restatement():
    c = chromosome()
    got = observed(c["sets"], c["records"])
    same(got, c["want"])
    st = got["stats"]
    assert st["slots"] == c["want"]["slots"].shape[0] and st["reads_counted"] < st["reads"] == c["want"]["first"].shape[0]
    assert st["observe_ms"] > 0 and st["link_ms"] > 0 and st["tag_ms"] > 0


def test_one_source_equals_the_restatement():
    c = chromosome()
    merged = reads_of_bam_records(sorted(c["short"] + c["long"], key=lambda r: r.pos))
    want = restatement([merged], c["records"])
    same(observed([merged], c["records"]), want)
    same(want, c["want"], PER_RECORD)                                                            # the reads of two BAMs count alike


def test_two_runs_give_the_same_bytes():
    c = chromosome()
    a, b = observed(c["sets"], c["records"]), observed(c["sets"], c["records"])
    for name in PER_READ + PER_RECORD:
        assert a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("max_span", [1000, None])
def test_spans_do_not_change_the_result(max_span, tmp_path):
    c = chromosome()
    paths = [str(tmp_path / "s.bam"), str(tmp_path / "l.bam")]
    for path, reads in zip(paths, (c["short"], c["long"])):
        write_bam(path, [("chr1", pc.LENGTH)], reads, index=True, block_bytes=20000)
    handles = [BamFile(p) for p in paths]
    try:
        stats = {}
        got = phase.chromosome_phase(handles, "chr1", pc.LENGTH, c["records"], window=pc.WINDOW, max_span=max_span, stats=stats)
        want = phase.chromosome_phase(handles, "chr1", pc.LENGTH, c["records"], window=pc.WINDOW, max_span=max_span, restatement=True)
    finally:
        for h in handles:
            h.close()
    same(got, want)
    same(got, c["want"], PER_RECORD)                                                             # whatever the spans
    assert stats["calls"] == (6 if max_span else 1) and stats["slots"] == c["want"]["slots"].shape[0]
    if max_span is None:
        same(got, c["want"])


# ---- (3) the driver -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["illumina", "hybrid"])
def test_call_phase_writes_the_restatements_file_and_leaves_the_others(kind, tmp_path):
    from hello_amd import candidates as cd
    from tests.test_gpu_candidates import _fasta, _write
    from tests.test_gpu_hybrid_candidates import synthetic as hybrid_synthetic
    from tests.test_gpu_resident import HYBRID_SEED, illumina_input
    from tests.util import load_fixture
    from hello_amd import loader, netspec as ns, weights
    hybrid = kind == "hybrid"
    if hybrid:
        reference, illumina, pacbio = hybrid_synthetic(HYBRID_SEED, 20000)
        bams = [_write(tmp_path, "i.bam", "chr1", reference, illumina), _write(tmp_path, "p.bam", "chr1", reference, pacbio)]
        route = ["--ibam", bams[0], "--pbam", bams[1], "--from_bams", "--resident", "--annotate_evidence"]
        thresholds = (10, 10)                                         # the driver's --q_threshold / --mapq_threshold defaults
    else:
        reference, reads = illumina_input()
        bams = [_write(tmp_path, "i.bam", "chr1", reference, reads)]
        route = ["--ibam", bams[0], "--from_bam"]
        thresholds = (cd.DEFAULT_Q_THRESHOLD, cd.DEFAULT_MIN_MAPQ)
    fa = _fasta(tmp_path, "chr1", reference)
    model = str(tmp_path / "model.hello.npz")
    if hybrid:
        loader.save_native(model, "hybrid_full", load_fixture("hybrid_full")[1])
    else:                                                             # synthetic weights of a seed that calls heterozygous genotypes here
        loader.save_native(model, "single_tech", weights.synth_state(ns.build("single_tech"), seed=MODEL_SEED))

    def run(extra, workdir):
        done = subprocess.run([sys.executable, "-m", "hello_amd.call", "--ref", fa, "--workdir", workdir, "--network", model] + route + extra,
                              cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-3000:]
    plain, phased = str(tmp_path / "w1"), str(tmp_path / "w2")
    run(["--gvcf"], plain)
    run(["--gvcf", "--phase"], phased)
    read = lambda *p: open(os.path.join(*p), "rb").read()      # noqa: E731
    for name in ("results.output.vcf", "results.output.g.vcf"):
        assert read(phased, name) == read(plain, name), name
    assert not os.path.exists(os.path.join(plain, "results.output.phased.vcf"))
    want = phase.write_phased_vcf(os.path.join(plain, "results.output.vcf"), bams, str(tmp_path / "want.vcf"), None, *thresholds,
                                  restatement=True)
    want_lines = open(want, "rb").read().splitlines(keepends=True)
    vcf_lines = read(plain, "results.output.vcf").splitlines(keepends=True)
    assert sum(phase.phasable(line) is not None for line in vcf_lines) >= 2                      # something to phase ...
    assert sum(b"|" in line.split(b"\t")[-1] for line in want_lines if not line.startswith(b"#")) >= 2     # ... and something phased
    assert len(want_lines) == len(vcf_lines) + 1
    assert read(phased, "results.output.phased.vcf") == b"".join(want_lines)
