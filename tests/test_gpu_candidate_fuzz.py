"""The hotspot and candidate kernels on the fuzz corpus of tests/candidate_fuzz.py: per route -- one Illumina
BAM, one PacBio BAM, both with ``hybrid_hotspot`` off and on -- over every seed, padded and unpadded, integer for integer against
the restatements, which tests/test_candidate_fuzz.py holds to an oracle that walks no CIGAR on the same inputs.  Then two checks
with no Python rule in them (shard by shard, resident gather), and the featurizer and the evidence kernel on the fuzz sites.
The reads go in as in-memory read sets; four seeds per route also go through BAM files and a FASTA with its lower-case stretch."""
import numpy as np
import pytest

from tests import candidate_fuzz as cf
from tests.bam_writer import write_bam

pytestmark = pytest.mark.gpu

CASES = [(route, pad) for route in cf.ROUTES for pad in (True, False)]
FILE_SEEDS = (0, 1, 2, 3)            # the seeds that also go through files, and whose sites go downstream
DOWNSTREAM = [("illumina", 0), ("pacbio", 0), ("two_bams", 0), ("two_bams", 1)]      # (route, technology)


def hotspots_of(route, reference, sets, span):
    from hello_amd import hotspots as hs
    return hs.find_positions(sets, reference, [span], pacbio=route == "pacbio", hybrid_hotspot=route == "hybrid",
                             q_threshold=cf.Q_THRESHOLD, mapq_threshold=cf.MAPQ_THRESHOLD)


def sites_of(route, reference, sets, positions, resident=False):
    from hello_amd import candidates as cd, hybrid
    from hello_amd.hotspots import HOTSPOTS_PACBIO
    if len(sets) == 2:
        return hybrid.find_sites(sets[0], sets[1], reference, positions, "chr", route == "hybrid", cf.REASSEMBLY_SIZE, cf.FEATURE_LENGTH,
                                 cf.Q_THRESHOLD, cf.MAPQ_THRESHOLD, resident=resident)
    return cd.find_sites(sets[0], reference, positions, "chr", cf.FEATURE_LENGTH, cf.Q_THRESHOLD, cf.MAPQ_THRESHOLD,
                         options=HOTSPOTS_PACBIO if route == "pacbio" else 0, resident=resident)


def same_payload(route, shard, sites, where):
    """``_same`` of tests/test_gpu_candidates.py and tests/test_gpu_hybrid_candidates.py: every payload array."""
    from hello_amd import shards
    if len(cf.profiles_of(route)) == 2:
        assert int(np.asarray(shard.z["has_second"]).reshape(-1)[0]) == 1 and shard.hybrid, where
        if not sites:
            assert shard.n_sites == 0 and all(np.asarray(shard.z[f"bases{t}"]).size == 0 for t in (0, 1)), where
            return
    want = shards._payload(cf.candidate_sites(route, sites))
    assert sorted(shard.z) == sorted(want), where
    for k in want:
        a, b = np.asarray(shard.z[k]), np.asarray(want[k])
        assert a.dtype == b.dtype or k == "has_second", where + (k,)
        assert np.array_equal(a.reshape(-1), b.reshape(-1)), where + (k,)


def same_bytes(a, b, where):
    for k in a.z:
        assert np.asarray(a.z[k]).tobytes() == np.asarray(b.z[k]).tobytes(), where + (k,)


@pytest.mark.parametrize("route,pad", CASES)
def test_hotspot_positions_and_plan_equal_the_restatement_and_two_runs_agree(route, pad):
    """All 32 seeds.  The positions and the statistics of the chunk plan, the tiles and the event capacity among them; a second
    run gives the same bytes."""
    flagged = 0
    for seed in cf.SEEDS:
        want = cf.restated(seed, route, pad)
        sets = [cf.read_set(rows) for rows in want["rows"]]
        span = cf.span_of(want["reference"], pad)
        got, st = hotspots_of(route, want["reference"], sets, span)
        assert got.tolist() == want["hotspots"], (route, pad, seed)
        assert {k: int(st[k]) for k in cf.HOTSPOT_STATS} == want["plan"], (route, pad, seed)
        again, _ = hotspots_of(route, want["reference"], sets, span)
        assert again.tobytes() == got.tobytes(), (route, pad, seed)
        flagged += got.shape[0]
    assert flagged > 0 or (not pad and route != "illumina")      # unpadded, the one 10 000-base chunk begins at 0 and is skipped


@pytest.mark.parametrize("route,pad", CASES)
def test_sites_regions_statistics_and_payload_equal_the_restatement_and_two_runs_agree(route, pad):
    """All 32 seeds.  ``regions_pass1``, ``regions_pass2``, every count statistic, every payload array of the shard and the read
    index; a second run gives the same bytes."""
    keys = [k for k in cf.stat_keys(route)]
    n_sites = 0
    for seed in cf.SEEDS:
        want = cf.restated(seed, route, pad)
        where = (route, pad, seed)
        sets = [cf.read_set(rows) for rows in want["site_rows"]]
        if seed == 0 and route != "illumina":                           # the PacBio read without a CIGAR is refused, loudly
            with pytest.raises(ValueError, match="no CIGAR operation on the reference"):
                sites_of(route, want["reference"], [cf.read_set(rows) for rows in want["rows"]], want["positions"])
        shard, st, extra = sites_of(route, want["reference"], sets, want["positions"])
        ws = want["stats"]
        assert extra["regions_pass1"].reshape(-1, 2).tolist() == [list(r) for r in ws["regions_pass1"]], where
        assert extra["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in ws["regions_pass2"]], where
        assert {k: int(st[k]) for k in keys} == {k: ws[k] for k in keys}, where
        same_payload(route, shard, want["sites"], where)
        for tech, index in enumerate(want["read_index"]):
            assert extra["read_index" + (str(tech) if len(sets) == 2 else "")].tolist() == index, where + (tech,)
        again, _, _ = sites_of(route, want["reference"], sets, want["positions"])
        same_bytes(shard, again, where)
        n_sites += shard.n_sites
    assert n_sites > (500 if pad else 100)


@pytest.mark.parametrize("route", cf.ROUTES)
def test_four_seeds_through_bam_files_and_a_fasta_with_a_lower_case_stretch(route, tmp_path):
    """The reference keeps its case here (80 lower-case bases mismatch every upper-case read base).  ``find_hotspots`` and the
    route's finder on files against the restatement on the same reads and reference."""
    from hello_amd import candidates as cd, hotspots as hs, hybrid, pacbio as pb
    from tests import candidate_reference as cr, hotspot_reference as hr, hybrid_reference as hy, pacbio_reference as pr
    for seed in FILE_SEEDS:
        reference, rows = cf.inputs(seed, route, True, True)
        assert reference != reference.upper()
        rows = [r if profile == "short" else [x for x in r if x[3]] for r, profile in zip(rows, cf.profiles_of(route))]
        reads = [cf.reads_of(r) for r in rows]
        paths = []
        for k, rs in enumerate(reads):
            paths.append(str(tmp_path / ("%s%d_%d.bam" % (route, seed, k))))
            write_bam(paths[-1], [("chrF", len(reference))], rs, index=True, block_bytes=20000)
        fa = str(tmp_path / ("%s%d.fa" % (route, seed)))
        with open(fa, "w") as fh:
            fh.write(">chrF fuzz\n" + "".join(reference[i:i + 60] + "\n" for i in range(0, len(reference), 60)))
        pacbio, hybrid_on = route == "pacbio", route == "hybrid"
        want = hr.find_hotspots(reads, reference, cf.START, len(reference), pacbio=pacbio, hybrid_hotspot=hybrid_on)
        got = hs.find_hotspots(paths if len(paths) == 2 else paths[0], fa, "chrF", cf.START, len(reference), pacbio=pacbio,
                               hybrid_hotspot=hybrid_on)
        assert got.tolist() == want and len(want) > 0, (route, seed)
        st, ws = {}, {}
        if route == "illumina":
            shard = cd.find_candidates(paths[0], fa, "chrF", want, stats=st)
            sites = cr.find_candidates(reads[0], reference, want, stats=ws)
        elif route == "pacbio":
            shard = pb.find_pacbio_candidates(paths[0], fa, "chrF", want, stats=st)
            sites = pr.find_candidates(reads[0], reference, want, stats=ws)
        else:
            shard = hybrid.find_hybrid_candidates(paths, fa, "chrF", want, hybrid_hotspot=hybrid_on, stats=st)
            sites = hy.find_candidates(reads[0], reads[1], reference, want, hybrid_on, stats=ws)
        assert st["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in ws["regions_pass2"]], (route, seed)
        assert {k: int(st[k]) for k in cf.stat_keys(route)} == {k: ws[k] for k in cf.stat_keys(route)}, (route, seed)
        from hello_amd import shards
        wanted = shards._payload(cf.candidate_sites(route, sites, "chrF"))
        for k in wanted:
            assert np.array_equal(np.asarray(shard.z[k]).reshape(-1), np.asarray(wanted[k]).reshape(-1)), (route, seed, k)


@pytest.mark.parametrize("route", cf.ROUTES)
def test_sites_found_shard_by_shard_equal_the_sites_found_at_once(route):
    """No Python rule: the hotspot positions cut by ``shard_positions`` into up to eight shards give, shard after shard, the
    arrays of the one call over all positions -- where the cut is neutral.  It is with a separation of 61: a location lies within
    15 bases of its positions, two locations less than 30 apart share a cluster, so positions 61 apart cannot (at the default 25
    two shards can split an active region, at 31 still a cluster, whose one fetch then clips other PacBio reads).  And not
    where pass 1 finds a location above 80 bases: ``cluster_locations`` drops it behind an open cluster and keeps it behind an
    empty one, which is what a shard's first location meets; those corpora are left out (what it found).  The 32
    padded corpora without the reads built on purpose, which plant such locations almost everywhere."""
    from hello_amd import candidates as cd
    compared = 0
    for seed in cf.SEEDS:
        want = cf.restated(seed, route, True, False)
        sets = [cf.read_set(rows) for rows in want["site_rows"]]
        whole, _, extra = sites_of(route, want["reference"], sets, want["positions"])
        pass1 = extra["regions_pass1"].reshape(-1, 2)
        if ((pass1[:, 1] - pass1[:, 0]) > 80).any():
            continue
        parts_of = cd.shard_positions(want["positions"], max_shards=8, min_separation=2 * cd.MIN_DISTANCE + 1)
        parts = [sites_of(route, want["reference"], sets, part)[0] for part in parts_of]
        joined = cd.concat_payloads(parts)
        for k in joined:
            if not k.startswith("chromosome"):
                assert np.array_equal(np.asarray(joined[k]).reshape(-1), np.asarray(whole.z[k]).reshape(-1)), (route, seed, k)
        compared += len(parts_of) >= 2
    assert compared >= 5, compared                      # as the census: at least five corpora per route (5 with two BAMs, 20 PacBio)


@pytest.mark.parametrize("route", cf.ROUTES)
def test_resident_gather_equals_the_host_gather(route):
    """No Python rule: ``hello_candidates_gather`` of the resident route against the arrays the host gathers, on the fuzz sites of
    the four seeds of FILE_SEEDS (guard bytes around every array)."""
    from tests.test_gpu_resident import gather, same_as_core
    for seed in FILE_SEEDS:
        want = cf.restated(seed, route, True)
        sets = [cf.read_set(rows) for rows in want["site_rows"]]
        plain, _, _ = sites_of(route, want["reference"], sets, want["positions"])
        resident, _, _ = sites_of(route, want["reference"], sets, want["positions"], resident=True)
        with resident:
            for tech in range(len(sets)):
                same_as_core(gather(resident, tech), plain, tech)


@pytest.fixture(scope="module")
def engine():
    from hello_amd import netspec as ns, weights
    from hello_amd.engine import Engine
    spec = ns.build("single_tech")
    eng = Engine(spec, weights.synth_state(spec, seed=5), device=0)
    yield eng
    eng.close()


def _shards(route):
    for seed in FILE_SEEDS[:2]:
        want = cf.restated(seed, route, True)
        sets = [cf.read_set(rows) for rows in want["site_rows"]]
        yield seed, sites_of(route, want["reference"], sets, want["positions"])[0]


@pytest.mark.parametrize("route,tech", DOWNSTREAM)
def test_featurizer_on_the_fuzz_sites_equals_its_oracle(engine, route, tech):
    """``featurize`` on the GPU shard's own arrays against ``oracle.featurizer_oracle`` read for read: clips, ``N``, ``P``, ``=`` /
    ``X`` and the clipped PacBio reads reach the featurizer here.  Two seeds per route (the oracle is a Python loop per base)."""
    from hello_amd.featurizer import featurize
    from oracle import featurizer_oracle as fo
    for seed, shard in _shards(route):
        a = shard.featurizer_arrays(tech)
        got, rpa, aps = featurize(engine, a, feature_length=cf.FEATURE_LENGTH)
        want, r = [], 0
        for allele, count in enumerate(a["reads_per_allele"].tolist()):
            site = int(a["site_of_read"][r])
            reads = []
            for k in range(r, r + count):
                words = a["cigars"][int(a["cigar_off"][k]):int(a["cigar_off"][k + 1])]
                lo, hi = int(a["read_off"][k]), int(a["read_off"][k + 1])
                if len(words):                                           # else the dummy read of an allele without support
                    reads.append(fo.Read(bytes(a["bases"][lo:hi]).decode(), a["quals"][lo:hi].tolist(), [(int(w) & 15, int(w) >> 4) for w in words],
                                         int(a["ref_start"][k]), int(a["mapq"][k]), int(a["orientation"][k]), int(a["hp"][k])))
            reference = bytes(a["ref"][int(a["ref_off"][site]):int(a["ref_off"][site + 1])]).decode()
            want.append(fo.features_for_reads(reads, reference, int(a["window_start"][site]), int(a["asm_start"][site]),
                                              int(a["asm_stop"][site]), cf.FEATURE_LENGTH, False))
            r += count
        want = np.concatenate(want, axis=0)
        assert got.shape == want.shape and (want != 0).any(), (route, tech, seed)
        bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
        assert bad.size == 0, (route, tech, seed, bad[:5].tolist())


@pytest.mark.parametrize("route,tech", DOWNSTREAM)
def test_allele_evidence_on_the_fuzz_sites_equals_the_python_loop(engine, route, tech):
    from hello_amd import featurizer as fz
    from tests.test_gpu_allele_evidence import python_evidence
    for seed, shard in _shards(route):
        a = shard.featurizer_arrays(tech)
        off = fz.allele_offsets(a["reads_per_allele"])
        want = python_evidence(a, off)
        got = fz.allele_evidence(engine, a, off)
        assert np.array_equal(got, want) and (want[:, :3].sum(axis=0) > 0).all(), (route, tech, seed)


@pytest.mark.parametrize("route", cf.ROUTES)
def test_the_hand_built_read_sets_of_the_lines_the_corpora_do_not_reach(route):
    """``candidate_fuzz.hand_built`` in every route (two BAMs: the same rows as either BAM): a region, a cluster and a site whose
    windows leave the chromosome, a position without reads, reads made right-partial by a trailing insertion, and events on the
    last and first column of a tile with flagged runs across the tile edge, a chunk edge and ``flag_lo - 1``."""
    for name in cf.hand_built():
        want = cf.hand_restated(route, name)
        ws = want["stats"]
        assert {k: ws[k] for k in cf.HAND_STATS[name]} == cf.HAND_STATS[name], (route, name)
        sets = [cf.read_set(rows) for rows in want["rows"]]
        got, _ = hotspots_of(route, want["reference"], sets, cf.HAND_SPAN)
        assert got.tolist() == want["hotspots"], (route, name)
        shard, st, extra = sites_of(route, want["reference"], sets, want["positions"])
        assert extra["regions_pass1"].reshape(-1, 2).tolist() == [list(r) for r in ws["regions_pass1"]], (route, name)
        assert extra["regions_pass2"].reshape(-1, 2).tolist() == [list(r) for r in ws["regions_pass2"]], (route, name)
        assert {k: int(st[k]) for k in cf.stat_keys(route)} == {k: ws[k] for k in cf.stat_keys(route)}, (route, name)
        same_payload(route, shard, want["sites"], (route, name))
