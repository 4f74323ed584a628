"""Genotype likelihoods and base-level evidence in the record lines (``--annotate_evidence``) on the CPU: the lines of
hello_site_records_evidence (hello_amd/csrc/records.hip) against the readable rules of hello_amd.vcf.annotate_evidence, byte
for byte, on the site tables of tests/test_annotate_records.py (one and two technologies, with and without the haplotag bit);
``PL`` on cases written out by hand; both strip round trips; the header for the four (technologies x hp) combinations; the
refusals; the flag."""
import ctypes
import os
import re

import numpy as np
import pytest

from hello_amd import call, records as R, vcf
from hello_amd.wrapper import pair_keys
from tests.test_annotate_records import GENOME, fields, hand_table, other
from tests.test_records import random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evidence_for(support, rng):
    """Evidence rows that fit ``support`` [A, 4]: nq <= reads, sums of nq values each, haplotag counts within the reads."""
    n = support[:, 0]
    nq = rng.integers(0, n + 1)
    nq[rng.random(n.shape[0]) < 0.2] = 0
    sum_q = np.array([rng.integers(0, 94, size=k).sum() for k in nq], np.int64)
    sum_d = np.array([rng.integers(0, 75, size=k).sum() for k in nq], np.int64)
    hp1 = rng.integers(0, n + 1)
    hp2 = rng.integers(0, n - hp1 + 1)
    return np.stack([nq, sum_q, sum_d, hp1, hp2, np.zeros_like(n)], axis=1).astype(np.int64)


def line_at(text, off, s):
    return bytes(text[off[s]:off[s + 1]]).decode()


@pytest.mark.parametrize("technologies,hp", [(1, False), (1, True), (2, False), (2, True)])
def test_hand_made_sites_equal_the_python_rules(technologies, hp):
    sites, table, post, support = hand_table()
    support = support[:technologies]
    rng = np.random.default_rng(5)
    evidence = [evidence_for(t, rng) for t in support]
    meta = np.tile(np.array([0.5, 0.25, 0.25], np.float32), (len(sites), 1))
    post = post.copy()
    post[2] *= 0.5                                                             # the mean row differs from the mixture row
    flags = R.HELLO_EVIDENCE_HP if hp else 0
    with R.site_records(table, post, meta, support=support, evidence=evidence, evidence_fields=flags) as rec, \
            R.site_records(table, post, meta, support=support) as annotated, R.site_records(table, post, meta) as plain:
        assert bytes(rec.features) == bytes(plain.features)
        col = a0 = lines = 0
        for s, (name, start, length, al, best, s0, s1, keep) in enumerate(sites):
            keys = pair_keys(al)
            rows = [dict(zip(keys, post[r, col:col + len(keys)].astype(np.float64).tolist())) for r in range(4)]
            col += len(keys)
            sup = [t[a0:a0 + len(al)] for t in support] + [None]
            evi = [t[a0:a0 + len(al)] for t in evidence] + [None]
            a0 += len(al)
            mean_row = vcf.mean_posteriors(rows[1:], meta[s])
            for got, old, older, row, info in (
                    (line_at(rec.shard_vcf, rec.shard_vcf_off, s), line_at(annotated.shard_vcf, annotated.shard_vcf_off, s),
                     line_at(plain.shard_vcf, plain.shard_vcf_off, s), rows[0], "MixtureOfExpertPrediction"),
                    (line_at(rec.mean_vcf, rec.mean_vcf_off, s), line_at(annotated.mean_vcf, annotated.mean_vcf_off, s),
                     line_at(plain.mean_vcf, plain.mean_vcf_off, s), mean_row, "HELLO")):
                c = vcf.call_site(row, "chr1", start, length, GENOME, info=info) if keep else None
                want = vcf.annotate_evidence(c, al, row, sup[0], evi[0], sup[1], evi[1], hp=hp) + "\n" if c else ""
                assert got == want, (name, info)
                assert vcf.strip_evidence(got) == old and vcf.strip_annotations(vcf.strip_evidence(got)) == older, (name, info)
                if c:
                    lines += 1
                    assert got.split("\t")[8] == vcf.evidence_format(technologies == 2, hp)
                    _, f = fields(got)
                    assert ("ADI" in f) == ("ADP" in f) == (technologies == 2) and ("AH1" in f) == ("AH2" in f) == hp
                    if technologies == 2:
                        both = [int(a) + int(b) for a, b in zip(f["ADI"].split(","), f["ADP"].split(","))]
                        assert both == [int(v) for v in f["AD"].split(",")]
        assert lines >= 2 * (len(sites) - 2)


@pytest.mark.parametrize("threads,technologies,hp", [(1, 1, True), (3, 2, False), (2, 2, True)])
def test_evidence_lines_equal_the_python_rules_on_random_sites(threads, technologies, hp):
    rng = np.random.default_rng(70 + threads)
    S = 500
    genome = "".join(rng.choice(list("ACGT"), size=S * 50 + 1000))
    names = ["chr1", "chrX"]
    aps, alleles, starts, stops, post, meta, chrom = random_table(rng, S, genome)
    post = post.copy()
    post[:, rng.random(post.shape[1]) < 0.1] = 0.0                            # posteriors of exactly 0
    keep = (rng.random(S) < 0.9).astype(np.uint8)
    A = int(aps.sum())
    support = []
    for _ in range(technologies):
        n = rng.integers(0, 40, size=A) * (rng.random(A) < 0.8)
        forward = rng.integers(0, n + 1)
        mapq = rng.integers(0, 256, size=A)
        support.append(np.stack([n, forward, n * mapq, n * mapq * mapq], axis=1).astype(np.int64))
    evidence = [evidence_for(t, rng) for t in support]
    text, off = R.text_table(np.array(alleles))
    table = R.SiteTable(aps, text, off, names, chrom, starts, stops, genomes={n: genome for n in names}, keep=keep)
    cuts = [0, 200, 200, S]
    flags = R.HELLO_EVIDENCE_HP if hp else 0
    seen = dict(lines=0, pl_absent=0, pl_six=0, pl_255=0, mbq_dot=0, mean_differs=0)
    with R.site_records(table, post, meta, shard_site_off=cuts, threads=threads, support=support, evidence=evidence,
                        evidence_fields=flags) as rec, \
            R.site_records(table, post, meta, shard_site_off=cuts, threads=threads, support=support) as annotated:
        assert bytes(rec.features) == bytes(annotated.features) and np.array_equal(rec.n_records, annotated.n_records)
        assert np.array_equal(rec.mean_position, annotated.mean_position) and np.array_equal(rec.qual, annotated.qual)
        col = a0 = 0
        for s in range(S):
            al = alleles[a0:a0 + aps[s]]
            sup = [t[a0:a0 + aps[s]] for t in support] + [None]
            evi = [t[a0:a0 + aps[s]] for t in evidence] + [None]
            a0 += aps[s]
            keys = pair_keys(al)
            rows = [dict(zip(keys, post[r, col:col + len(keys)].astype(np.float64).tolist())) for r in range(4)]
            col += len(keys)
            start, length = int(starts[s]), int(stops[s] - starts[s])
            c = vcf.call_site(rows[0], names[chrom[s]], start, length, genome, info="MixtureOfExpertPrediction") if keep[s] else None
            got = line_at(rec.shard_vcf, rec.shard_vcf_off, s)
            assert got == (vcf.annotate_evidence(c, al, rows[0], sup[0], evi[0], sup[1], evi[1], hp=hp) + "\n" if c else ""), s
            assert vcf.strip_evidence(got) == line_at(annotated.shard_vcf, annotated.shard_vcf_off, s), s
            got_mean = line_at(rec.mean_vcf, rec.mean_vcf_off, s)
            if c is None:
                assert got_mean == ""
                continue
            mean_row = vcf.mean_posteriors(rows[1:], meta[s])
            mean = vcf.call_site(mean_row, names[chrom[s]], start, length, genome)
            assert got_mean == (vcf.annotate_evidence(mean, al, mean_row, sup[0], evi[0], sup[1], evi[1], hp=hp) + "\n" if mean else ""), s
            assert vcf.strip_evidence(got_mean) == line_at(annotated.mean_vcf, annotated.mean_vcf_off, s), s
            info, f = fields(got)
            seen["lines"] += 1
            seen["pl_absent"] += f["PL"] == "."
            seen["pl_six"] += f["PL"].count(",") == 5
            seen["pl_255"] += "255" in f["PL"].split(",")
            seen["mbq_dot"] += "." in info.split(";MBQ=")[1].split(";")[0].split(",")
            seen["mean_differs"] += bool(mean) and fields(got_mean)[1]["PL"] != f["PL"]
            if f["PL"] != ".":                                              # the called genotype's PL is 0
                g = sorted(int(x) for x in f["GT"].split("/"))
                assert f["PL"].split(",")[g[1] * (g[1] + 1) // 2 + g[0]] == "0", s
    assert all(v > 0 for v in seen.values()), seen


# ---- PL by hand ---------------------------------------------------------------------------------------------------------
def library_line(alleles, start, length, row, support_rows=None, evidence_rows=None):
    """The shard line of ONE site whose mixture row is ``row`` ({pair: p}), through hello_site_records_evidence."""
    keys = pair_keys(alleles)
    post = np.zeros((4, len(keys)), np.float32)
    for k, key in enumerate(keys):
        post[:, k] = row[key] if key in row else row[key[::-1]]
    text, off = R.text_table(np.array(alleles))
    table = R.SiteTable(np.array([len(alleles)], np.int32), text, off, ["chr1"], np.zeros(1, np.int32), [start], [start + length],
                        genomes={"chr1": GENOME})
    support = np.array(support_rows or [(2, 1, 120, 7200)] * len(alleles), np.int64)
    evidence = np.array(evidence_rows or [(2, 60, 20, 0, 0, 0)] * len(alleles), np.int64)
    with R.site_records(table, post, None, support=[support], evidence=[evidence]) as rec:
        line = line_at(rec.shard_vcf, rec.shard_vcf_off, 0)
    exact = {key: float(np.float32(row[key] if key in row else row[key[::-1]])) for key in keys}
    c = vcf.call_site(exact, "chr1", start, length, GENOME, info="MixtureOfExpertPrediction")
    assert line == vcf.annotate_evidence(c, alleles, exact, support, evidence) + "\n"
    return line


def test_pl_by_hand():
    r = GENOME[1500]
    a, b = other(r), other(r, 2)
    # het: p(ref/ref) = 0.01, p(ref/alt) = 0.9, p(alt/alt) = 0.09: -10 log10(0.01 / 0.9) = 19.54 -> 20, 0, -10 log10(0.1) = 10
    _, f = fields(library_line([r, a], 1500, 1, {(r, r): 0.01, (r, a): 0.9, (a, a): 0.09}))
    assert (f["GT"], f["PL"]) == ("0/1", "20,0,10")
    # hom-alt: 0.0009 / 0.9 -> 30, 0.09 / 0.9 -> 10, 0
    _, f = fields(library_line([r, a], 1500, 1, {(r, r): 0.0009, (r, a): 0.09, (a, a): 0.9}))
    assert (f["GT"], f["PL"]) == ("1/1", "30,10,0")
    # hom-ref listing two ALTs: six values in VCF order 00, 01, 11, 02, 12, 22 (ALTs in the record's sorted order)
    first, second = sorted([a, b])
    row = {(r, r): 0.8, (r, first): 0.08, (first, first): 0.008, (r, second): 0.0008, (first, second): 0.00008, (second, second): 0.04}
    line = library_line([r, a, b], 1500, 1, row)
    _, f = fields(line)
    assert line.split("\t")[4] == first + "," + second and (f["GT"], f["PL"]) == ("0/0", "0,10,20,30,40,13")
    # a posterior of exactly 0 -> 255, and a tiny one is capped at 255 as well
    _, f = fields(library_line([r, a], 1500, 1, {(r, r): 0.0, (r, a): 0.9, (a, a): 1e-30}))
    assert (f["GT"], f["PL"]) == ("0/1", "255,0,255")
    # 254.5 rounds to 255, 254.4 stays 254 (the cap is applied after the rounding)
    _, f = fields(library_line([r, a], 1500, 1, {(r, r): 10 ** -25.44, (r, a): 1.0, (a, a): 10 ** -25.46}))
    assert f["PL"] == "254,0,255"
    # the reference allele is not among the site's alleles -> the whole field is `.`
    line = library_line([a, b], 1500, 1, {(a, a): 0.9, (a, b): 0.05, (b, b): 0.05})
    info, f = fields(line)
    assert (f["GT"], f["PL"], f["AD"]) == ("1/1", ".", "0,2") and info.endswith(";MBQ=.,30;MPOS=.,10")
    # every posterior 0: p_max <= 0 -> `.`
    _, f = fields(library_line([r, a], 1500, 1, {(r, r): 0.0, (r, a): 0.0, (a, a): 0.0}))
    assert f["PL"] == "."


def test_mbq_and_mpos_round_half_up_and_sum_the_technologies():
    c = vcf.Call("chr1", 9, "A", ("C", "G"), (0, 1), 30.0, source=("A", "C", "G"))
    post = {("A", "A"): 0.05, ("A", "C"): 0.9, ("C", "C"): 0.05, ("A", "G"): 0.0, ("C", "G"): 0.0, ("G", "G"): 0.0}
    support0, support1 = [(4, 2, 240, 14400), (2, 1, 120, 7200), (0, 0, 0, 0)], [(1, 1, 60, 3600), (3, 0, 180, 10800), (0, 0, 0, 0)]
    evidence0 = [(3, 91, 10, 1, 2, 0), (2, 61, 7, 0, 2, 0), (0, 0, 0, 0, 0, 0)]      # 91 / 3 = 30.33, 61 / 2 = 30.5, 7 / 2 = 3.5
    evidence1 = [(1, 37, 5, 1, 0, 0), (0, 0, 0, 3, 0, 0), (0, 0, 0, 0, 0, 0)]        # (91 + 37) / 4 = 32, (10 + 5) / 4 = 3.75
    line = vcf.annotate_evidence(c, ["A", "C", "G"], post, support0, evidence0, support1, evidence1, hp=True)
    assert line == ("chr1\t10\t.\tA\tC,G\t30.000000\tPASS\tHELLO;MQ=60.00;MBQ=32,31,.;MPOS=4,4,.\t"
                    "GT:GQ:DP:AD:ADF:ADR:PL:ADI:ADP:AH1:AH2\t0/1:30:10:5,5,0:3,1,0:2,4,0:13,0,13,255,255,255:4,2,0:1,3,0:2,3,0:2,2,0")
    assert vcf.strip_evidence(line) == vcf.annotate(c, ["A", "C", "G"], support0, support1)
    assert vcf.strip_annotations(vcf.strip_evidence(line)) == c.line()
    assert vcf.strip_evidence(c.line()) == c.line() and vcf.strip_evidence(vcf.strip_evidence(line) + "\n") == vcf.strip_evidence(line) + "\n"
    one = vcf.annotate_evidence(c, ["A", "C", "G"], post, support0, evidence0)
    assert one.split("\t")[7:9] == ["HELLO;MQ=60.00;MBQ=30,31,.;MPOS=3,4,.", "GT:GQ:DP:AD:ADF:ADR:PL"]
    with pytest.raises(ValueError, match="evidence1 goes with support1"):
        vcf.annotate_evidence(c, ["A", "C", "G"], post, support0, evidence0, support1)


@pytest.mark.parametrize("two,hp", [(False, False), (False, True), (True, False), (True, True)])
def test_header_gains_one_declaration_per_field_written(two, hp):
    plain = call.header(["chr1"], {"chr1": 10})
    got = call.header(["chr1"], {"chr1": 10}, annotate=True, evidence=(two, hp))
    assert got == call.header(["chr1"], {"chr1": 10}, evidence=(two, hp))                     # the flag implies --annotate's fields
    added = [line for line in got.splitlines() if line not in plain.splitlines()]
    assert "".join(line + "\n" for line in added) == vcf.evidence_header(two, hp)
    want = [("INFO", "MQ", "1"), ("FORMAT", "GQ", "1"), ("FORMAT", "DP", "1"), ("FORMAT", "AD", "R"), ("FORMAT", "ADF", "R"),
            ("FORMAT", "ADR", "R"), ("INFO", "MBQ", "R"), ("INFO", "MPOS", "R"), ("FORMAT", "PL", "G")]
    want += [("FORMAT", "ADI", "R"), ("FORMAT", "ADP", "R")] if two else []
    want += [("FORMAT", "AH1", "R"), ("FORMAT", "AH2", "R")] if hp else []
    assert [re.match(r"##(INFO|FORMAT)=<ID=(\w+),Number=(\w),Type=\w+,Description=\"[^\"]+\">$", line).groups() for line in added] == want
    declared = {w[1] for w in want if w[0] == "FORMAT"} | {"GT"}
    assert set(vcf.evidence_format(two, hp).split(":")) == declared                          # every written field, and no other
    assert [line for line in got.splitlines() if line in plain.splitlines()] == plain.splitlines()
    assert got.splitlines()[-1].startswith("#CHROM")
    assert call.header(["chr1"], {"chr1": 10}, annotate=True) == plain.replace("#CHROM", vcf.ANNOTATION_HEADER + "#CHROM")


def test_refusals():
    bound = R._lib()
    sites, table, post, support = hand_table()
    evidence = [evidence_for(t, np.random.default_rng(1)) for t in support]
    out = ctypes.c_void_p()

    def run(s0, s1, e0, e1, flags=0):
        ptr = lambda a: a.ctypes.data if a is not None else None                # noqa: E731
        return bound.hello_site_records_evidence(ctypes.byref(table.struct), ptr(s0), ptr(s1), ptr(e0), ptr(e1), flags, post.ctypes.data,
                                                 post.shape[1], None, None, 1, None, 0, ctypes.byref(out))
    assert run(support[0], support[1], evidence[0], None) == -1 and b"evidence1 must be NULL exactly when support1" in bound.hello_last_error()
    assert run(support[0], None, evidence[0], evidence[1]) == -1 and b"evidence1 must be NULL exactly when support1" in bound.hello_last_error()
    assert run(support[0], None, None, None) == -1 and b"evidence0" in bound.hello_last_error()
    assert run(None, None, evidence[0], None) == -1
    assert run(support[0], None, evidence[0], None, flags=2) == -1 and b"unknown bit" in bound.hello_last_error()
    assert out.value is None
    assert run(support[0], None, evidence[0], None, flags=R.HELLO_EVIDENCE_HP) == 0 and out.value
    bound.hello_records_destroy(out)
    with pytest.raises(ValueError, match="one int64 .* array per technology"):
        R.site_records(table, post, None, support=support, evidence=evidence[:1])
    with pytest.raises(ValueError, match="one int64 .* array per technology"):
        R.site_records(table, post, None, support=support[:1], evidence=[evidence[0][:, :4]])
    with pytest.raises(ValueError, match="evidence goes with support"):
        R.site_records(table, post, None, evidence=evidence)


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd import featurizer, shard_pipeline as sp
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_engine_allele_evidence", "hello_site_records_evidence"):
        assert re.search(r"\bint %s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert int(re.search(r"#define HELLO_ABI_VERSION (\d+)", header).group(1)) == lib.hello_abi_version() == 2          # additions only
    assert int(re.search(r"#define HELLO_EVIDENCE_HP (\d+)", header).group(1)) == R.HELLO_EVIDENCE_HP
    assert len(lib.hello_engine_allele_evidence.argtypes) == 17
    assert featurizer.EVIDENCE_ARRAYS == ("quals", "read_off", "cigars", "cigar_off", "ref_start", "hp", "site_of_read", "asm_start",
                                          "asm_stop", "allele_off")
    assert len(R._lib().hello_site_records_evidence.argtypes) == len(R._lib().hello_site_records_annotated.argtypes) + 3
    # without a GPU: a NULL engine is refused with HELLO_ERR_ARG
    assert lib.hello_engine_allele_evidence(*([None] * 11), 0, 0, 0, None, 0, None) == -1 and b"engine is NULL" in lib.hello_last_error()
    scored = sp.Scored([], [], np.zeros((4, 0), np.float32), None)
    assert scored.evidence is None and scored.evidence_fields == 0
    assert "evidence" in sp.ShardScorer.__init__.__code__.co_varnames and "evidence" in call.score_shard.__code__.co_varnames
    assert "evidence" in sp.run.__code__.co_varnames


def test_the_flag_parses_and_is_forwarded_to_the_ranks():
    base = ["--workdir", "w", "--network", "m.npz", "--shards", "s"]
    args = call.parser().parse_args(base + ["--annotate_evidence"])
    assert args.annotate_evidence and not args.annotate and not call.parser().parse_args(base + ["--annotate"]).annotate_evidence
    assert "--annotate_evidence" in call._argv_of(call.parser().parse_args(base + ["--annotate_evidence", "--gpus", "4"]))
    assert "--annotate_evidence" not in call._argv_of(call.parser().parse_args(base + ["--annotate"]))
    assert "--include_hp" in call._argv_of(call.parser().parse_args(base + ["--annotate_evidence", "--include_hp"]))
