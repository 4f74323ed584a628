"""Read support in the record lines (``--annotate``) on the CPU: the lines of hello_site_records_annotated
(hello_amd/csrc/records.hip) against the readable rules of hello_amd.vcf.annotate, byte for byte, on hand-made sites that name
every rule and on seeded random sites; the same lines without their annotations against hello_site_records; the header lines,
the flag and the two ABI symbols.

QUAL tops out at 80.0000000264 in this record stage (p is capped at 1 - 1e-8, prepareVcf.py:61), so no line of the library can
carry a QUAL above 99: the cap of GQ at 99 is held on the restatement with a hand-made call, and the library's largest QUAL is
held to GQ = 80."""
import ctypes
import os
import re

import numpy as np
import pytest

from hello_amd import call, records as R, vcf
from hello_amd.wrapper import pair_keys
from tests.test_records import random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = "".join(np.random.default_rng(3).choice(list("ACGT"), size=4000))


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def hand_sites():
    """-> [(name, start, length, alleles, best pair, support0 rows, support1 rows, keep)].  Rows: (reads, forward, sum mapq, sum mapq^2)."""
    g, out = GENOME, []

    def row(mapqs, forward):
        return (len(mapqs), forward, sum(mapqs), sum(q * q for q in mapqs))
    r = g[100]
    out.append(("the reference allele is not among the site's alleles", 100, 1, [other(r), other(r, 2)], (other(r), other(r)),
                [row([60, 60, 20], 2), row([10], 0)], [row([], 0), row([], 0)], 1))
    r = g[200]
    out.append(("hom-ref listing two ALTs", 200, 1, [other(r, 2), r, other(r)], (r, r),
                [row([60], 1), row([60] * 7, 3), row([0, 1], 2)], [row([255], 0), row([30, 30], 1), row([], 0)], 1))
    r = g[300]
    out.append(("1/2", 300, 1, [r, other(r), other(r, 3)], (other(r), other(r, 3)),
                [row([60], 1), row([60] * 5, 2), row([60] * 4, 4)], [row([], 0), row([50], 1), row([40, 40], 0)], 1))
    at = next(i for i in range(400, 900) if g[i + 1] != g[i] and g[i - 1] != g[i])
    r = g[at:at + 2]                  # XY -> Y: the shared Y is trimmed, the emptied ALT re-anchors on the base before
    out.append(("an indel whose normalisation trims and re-anchors", at, 2, [r, r[1]], (r, r[1]),
                [row([60] * 6, 3), row([60, 59, 58], 1)], [row([20], 1), row([], 0)], 1))
    r = g[1000]
    out.append(("an ALT with zero support, and reads on an allele the record does not list", 1000, 1, [r, other(r), other(r, 2)],
                (r, other(r)), [row([60] * 9, 4), row([], 0), row([33, 34, 35], 3)], [row([], 0), row([], 0), row([1], 0)], 1))
    r = g[1100]
    out.append(("keep = 0", 1100, 1, [r, other(r)], (r, other(r)), [row([60], 1), row([60], 0)], [row([], 0), row([], 0)], 0))
    r = g[1200]
    out.append(("the largest QUAL", 1200, 1, [r, other(r)], (other(r), other(r)), [row([60], 1), row([60, 60], 0)],
                [row([60], 1), row([], 0)], 1))
    r = g[1300]
    out.append(("no read at all", 1300, 1, [r, other(r)], (r, other(r)), [row([], 0), row([], 0)], [row([], 0), row([], 0)], 1))
    return out


def hand_table():
    sites = hand_sites()
    aps = np.array([len(s[3]) for s in sites], np.int32)
    alleles = [a for s in sites for a in s[3]]
    P = int((aps * (aps + 1) // 2).sum())
    post = np.zeros((4, P), np.float32)
    col = 0
    for name, start, length, al, best, s0, s1, keep in sites:
        keys = pair_keys(al)
        post[:, col:col + len(keys)] = 0.01
        k = keys.index(best) if best in keys else keys.index(best[::-1])
        post[:, col + k] = 1.0 if name == "the largest QUAL" else 0.9
        col += len(keys)
    text, off = R.text_table(np.array(alleles))
    table = R.SiteTable(aps, text, off, ["chr1"], np.zeros(len(sites), np.int32), [s[1] for s in sites], [s[1] + s[2] for s in sites],
                        genomes={"chr1": GENOME}, keep=np.array([s[7] for s in sites], np.uint8))
    support = [np.array([r for s in sites for r in s[5]], np.int64), np.array([r for s in sites for r in s[6]], np.int64)]
    return sites, table, post, support


def fields(line):
    """An annotated line -> (INFO, {FORMAT key: value})."""
    cols = line.rstrip("\n").split("\t")
    return cols[7], dict(zip(cols[8].split(":"), cols[9].split(":")))


def test_hand_made_sites_carry_the_stated_values():
    sites, table, post, support = hand_table()
    meta = np.tile(np.array([1, 0, 0], np.float32), (len(sites), 1))
    with R.site_records(table, post, meta, support=support) as rec, R.site_records(table, post, meta) as plain:
        got = {}
        col = a0 = 0
        for s, (name, start, length, al, best, s0, s1, keep) in enumerate(sites):
            keys = pair_keys(al)
            row = dict(zip(keys, post[0, col:col + len(keys)].astype(np.float64).tolist()))
            col += len(keys)
            for text, off, old, old_off, info in ((rec.shard_vcf, rec.shard_vcf_off, plain.shard_vcf, plain.shard_vcf_off, "MixtureOfExpertPrediction"),
                                                  (rec.mean_vcf, rec.mean_vcf_off, plain.mean_vcf, plain.mean_vcf_off, "HELLO")):
                line = bytes(text[off[s]:off[s + 1]]).decode()
                c = vcf.call_site(row, "chr1", start, length, GENOME, info=info) if keep else None
                want = vcf.annotate(c, al, support[0][a0:a0 + len(al)], support[1][a0:a0 + len(al)]) + "\n" if c else ""
                assert line == want, (name, info)
                assert vcf.strip_annotations(line) == bytes(old[old_off[s]:old_off[s + 1]]).decode() == (c.line() + "\n" if c else ""), name
            got[name] = bytes(rec.shard_vcf[rec.shard_vcf_off[s]:rec.shard_vcf_off[s + 1]]).decode()
            a0 += len(al)
        assert bytes(rec.features) == bytes(plain.features)                      # the .features streams do not change

    info, f = fields(got["the reference allele is not among the site's alleles"])
    assert (f["GT"], f["DP"], f["AD"], f["ADF"], f["ADR"]) == ("1/1", "4", "0,3", "0,2", "0,1")
    assert info == "MixtureOfExpertPrediction;MQ=%.2f" % np.sqrt((60 * 60 * 2 + 400 + 100) / 4)
    info, f = fields(got["hom-ref listing two ALTs"])                         # ALTs sorted: the order of the record, not of the site
    site = hand_sites()[1]
    order = [site[3].index(site[3][1])] + [site[3].index(a) for a in sorted(x for x in site[3] if x != site[3][1])]
    both = np.array(site[5]) + np.array(site[6])
    assert f["GT"] == "0/0" and f["DP"] == "13" and f["AD"] == ",".join(str(both[i][0]) for i in order)
    assert f["ADF"] == ",".join(str(both[i][1]) for i in order) and f["ADR"] == ",".join(str(both[i][0] - both[i][1]) for i in order)
    info, f = fields(got["1/2"])
    assert f["GT"] in ("1/2", "2/1") and f["DP"] == "13" and f["AD"].split(",")[0] == "1" and sorted(f["AD"].split(",")[1:]) == ["6", "6"]
    line = got["an indel whose normalisation trims and re-anchors"]
    site = hand_sites()[3]
    cols = line.split("\t")
    assert int(cols[1]) == site[1] and (cols[3], cols[4]) == (GENOME[site[1] - 1:site[1] + 1], GENOME[site[1] - 1])    # moved one base left
    info, f = fields(line)
    assert (f["GT"], f["DP"], f["AD"], f["ADF"], f["ADR"]) == ("0/1", "10", "7,3", "4,1", "3,2")
    info, f = fields(got["an ALT with zero support, and reads on an allele the record does not list"])
    assert (f["GT"], f["DP"], f["AD"], f["ADF"], f["ADR"]) == ("0/1", "13", "9,0", "4,0", "5,0")          # DP > sum(AD)
    assert got["keep = 0"] == ""
    info, f = fields(got["the largest QUAL"])
    assert got["the largest QUAL"].split("\t")[5] == "80.000000" and f["GQ"] == "80" and f["DP"] == "4" and info.endswith(";MQ=60.00")
    info, f = fields(got["no read at all"])
    assert info == "MixtureOfExpertPrediction;MQ=." and (f["DP"], f["AD"], f["ADF"], f["ADR"]) == ("0", "0,0", "0,0", "0,0")
    assert f["GQ"] == "10"                                                      # -10 log10(1 - 0.9) = 10


def test_genotype_quality_is_capped_at_99_in_the_restatement():
    c = vcf.Call("chr1", 9, "A", ("C",), (0, 1), 120.3, source=("A", "C"))
    line = vcf.annotate(c, ["A", "C"], [(3, 1, 180, 10800), (2, 2, 120, 7200)])
    assert line == "chr1\t10\t.\tA\tC\t120.300000\tPASS\tHELLO;MQ=60.00\tGT:GQ:DP:AD:ADF:ADR\t0/1:99:5:3,2:1,2:2,0"
    assert vcf.strip_annotations(line) == c.line()
    for qual, gq in ((98.49, 98), (98.5, 99), (99.5, 99), (0.49, 0), (0.5, 1)):
        c.qual = qual
        assert fields(vcf.annotate(c, ["A", "C"], [(0, 0, 0, 0)] * 2))[1]["GQ"] == str(gq)


@pytest.mark.parametrize("threads,technologies", [(1, 1), (3, 2)])
def test_annotated_lines_equal_the_python_rules_on_random_sites(threads, technologies):
    rng = np.random.default_rng(40 + threads)
    S = 700
    genome = "".join(rng.choice(list("ACGT"), size=S * 50 + 1000))
    names = ["chr1", "chrX"]
    aps, alleles, starts, stops, post, meta, chrom = random_table(rng, S, genome)
    keep = (rng.random(S) < 0.9).astype(np.uint8)
    A = int(aps.sum())
    support = []
    for _ in range(technologies):
        n = rng.integers(0, 40, size=A) * (rng.random(A) < 0.8)
        forward = rng.integers(0, n + 1)
        mapq = rng.integers(0, 256, size=A)
        support.append(np.stack([n, forward, n * mapq, n * mapq * mapq], axis=1).astype(np.int64))
    site_of = np.repeat(np.arange(S), aps)
    empty = rng.random(S) < 0.05                                             # sites without a read in any technology
    for t in support:
        t[empty[site_of]] = 0
    text, off = R.text_table(np.array(alleles))
    table = R.SiteTable(aps, text, off, names, chrom, starts, stops, genomes={n: genome for n in names}, keep=keep)
    cuts = [0, 300, 300, S]
    seen = dict(lines=0, absent_ref=0, hom_ref_two=0, het_alt=0, moved=0, unlisted=0, no_reads=0)
    with R.site_records(table, post, meta, shard_site_off=cuts, threads=threads, support=support) as rec, \
            R.site_records(table, post, meta, shard_site_off=cuts, threads=threads) as plain:
        assert bytes(rec.features) == bytes(plain.features) and np.array_equal(rec.n_records, plain.n_records)
        assert np.array_equal(rec.mean_position, plain.mean_position) and np.array_equal(rec.qual, plain.qual)
        col = a0 = 0
        for s in range(S):
            al = alleles[a0:a0 + aps[s]]
            sup = [t[a0:a0 + aps[s]] for t in support] + [None]
            a0 += aps[s]
            keys = pair_keys(al)
            rows = [dict(zip(keys, post[r, col:col + len(keys)].astype(np.float64).tolist())) for r in range(4)]
            col += len(keys)
            start, length = int(starts[s]), int(stops[s] - starts[s])
            c = vcf.call_site(rows[0], names[chrom[s]], start, length, genome, info="MixtureOfExpertPrediction") if keep[s] else None
            got = bytes(rec.shard_vcf[rec.shard_vcf_off[s]:rec.shard_vcf_off[s + 1]]).decode()
            assert got == (vcf.annotate(c, al, sup[0], sup[1]) + "\n" if c else ""), s
            assert vcf.strip_annotations(got) == bytes(plain.shard_vcf[plain.shard_vcf_off[s]:plain.shard_vcf_off[s + 1]]).decode(), s
            got_mean = bytes(rec.mean_vcf[rec.mean_vcf_off[s]:rec.mean_vcf_off[s + 1]]).decode()
            if c is None:
                assert got_mean == ""
                continue
            mean = vcf.call_site(vcf.mean_posteriors(rows[1:], meta[s]), names[chrom[s]], start, length, genome)
            assert got_mean == (vcf.annotate(mean, al, sup[0], sup[1]) + "\n" if mean else ""), s
            assert vcf.strip_annotations(got_mean) == bytes(plain.mean_vcf[plain.mean_vcf_off[s]:plain.mean_vcf_off[s + 1]]).decode(), s
            _, f = fields(got)
            ad = [int(v) for v in f["AD"].split(",")]
            seen["lines"] += 1
            seen["absent_ref"] += genome[start:start + length] not in al
            seen["hom_ref_two"] += f["GT"] == "0/0" and len(ad) == 3
            seen["het_alt"] += f["GT"] in ("1/2", "2/1")
            seen["moved"] += c.position != start
            seen["unlisted"] += int(f["DP"]) > sum(ad)
            seen["no_reads"] += f["DP"] == "0"
    assert all(v > 0 for v in seen.values()), seen                           # the sweep reaches every rule as well


def test_header_lines_appear_only_with_annotate():
    plain, annotated = call.header(["chr1"], {"chr1": 10}), call.header(["chr1"], {"chr1": 10}, annotate=True)
    assert plain == call.header(["chr1"], {"chr1": 10}, annotate=False) and "MQ" not in plain and "ID=DP" not in plain
    added = [line for line in annotated.splitlines() if line not in plain.splitlines()]
    assert [re.match(r"##(INFO|FORMAT)=<ID=(\w+),Number=(\w)", line).groups() for line in added] == [
        ("INFO", "MQ", "1"), ("FORMAT", "GQ", "1"), ("FORMAT", "DP", "1"), ("FORMAT", "AD", "R"), ("FORMAT", "ADF", "R"), ("FORMAT", "ADR", "R")]
    assert [line for line in annotated.splitlines() if line in plain.splitlines()] == plain.splitlines()
    assert annotated.splitlines()[-1].startswith("#CHROM")


def test_the_flag_parses_and_is_forwarded_to_the_ranks():
    base = ["--workdir", "w", "--network", "m.npz", "--shards", "s"]
    assert call.parser().parse_args(base + ["--annotate"]).annotate and not call.parser().parse_args(base).annotate
    assert "--annotate" in call._argv_of(call.parser().parse_args(base + ["--annotate", "--gpus", "4"]))
    assert "--annotate" not in call._argv_of(call.parser().parse_args(base))


def test_abi_symbols_are_declared_exported_and_mirrored():
    from hello_amd import featurizer, shard_pipeline as sp
    from hello_amd.engine import load_library
    header = open(os.path.join(ROOT, "include", "hello_mi355x.h")).read()
    lib = load_library()
    for symbol in ("hello_engine_allele_support", "hello_site_records_annotated"):
        assert re.search(r"\bint %s\(" % symbol, header), symbol
        assert hasattr(lib, symbol), symbol
    assert int(re.search(r"#define HELLO_ABI_VERSION (\d+)", header).group(1)) == lib.hello_abi_version() == 2          # additions only
    assert len(lib.hello_engine_allele_support.argtypes) == 10 and featurizer.SUPPORT_ARRAYS == ("cigar_off", "mapq", "orientation", "allele_off")
    bound = R._lib()
    assert len(bound.hello_site_records_annotated.argtypes) == len(bound.hello_site_records.argtypes) + 2
    # without a GPU: NULL arguments are refused with HELLO_ERR_ARG
    assert lib.hello_engine_allele_support(None, None, None, None, None, 0, 0, None, 0, None) == -1 and b"engine is NULL" in lib.hello_last_error()
    sites, table, post, support = hand_table()
    out = ctypes.c_void_p()
    assert bound.hello_site_records_annotated(ctypes.byref(table.struct), None, None, post.ctypes.data, post.shape[1], None, None, 1, None,
                                              0, ctypes.byref(out)) == -1 and b"support0" in bound.hello_last_error()
    with pytest.raises(ValueError, match="one or two int64"):
        R.site_records(table, post, None, support=[support[0][:-1]])
    assert sp.Scored([], [], post, None).support is None
    assert "annotate" in sp.ShardScorer.__init__.__code__.co_varnames and "annotate" in call.score_shard.__code__.co_varnames
