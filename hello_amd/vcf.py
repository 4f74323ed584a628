"""Genotype calls and VCF records from pair posteriors.

What the reference does with the network's output, per site:
  * per-shard caller: best unordered allele pair -> QUAL = -10 log10(1 - p) capped at p = 1 - 1e-8,
    genotype indices against the ALT list, one normalised VCF line
    (reference python/caller_calling.py:698-743, python/vcfFromContigs.py:139-227);
  * final VCF: the same on the meta-weighted mean of the three experts' posteriors
    (python/prepareVcf.py:36-105,138-168).

ALT alleles are emitted in sorted order (the reference's order is ``list(set(...))``, i.e. Python's
per-process hash order; SURVEY.md section 7 defines call identity on the ALT *set*).  Everything here is
string work on the host; the posteriors themselves come from the GPU (hello_amd.wrapper).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

QUAL_CAP = 1 - 1e-8            # "Quality score restricted to value 80" (prepareVcf.py:61)


@dataclass
class Call:
    chromosome: str
    position: int               # 0-based, after normalisation
    ref: str
    alts: Tuple[str, ...]
    genotype: Tuple[int, int]
    qual: float
    info: str = "HELLO"
    filter: str = "PASS"
    # the reference allele and the ALTs as the site spells them, BEFORE normalisation (what ``annotate`` looks up); not part
    # of a call's value
    source: Tuple[str, ...] = field(default=(), compare=False, repr=False)

    def line(self) -> str:
        return "%s\t%d\t.\t%s\t%s\t%f\t%s\t%s\tGT\t%s" % (
            self.chromosome, self.position + 1, self.ref, ",".join(self.alts), self.qual, self.filter,
            self.info, "/".join(str(g) for g in self.genotype))

    def identity(self):
        """What two pipelines must agree on for a call to count as identical."""
        alleles = (self.ref,) + self.alts
        return (self.chromosome, self.position, self.ref, frozenset(self.alts),
                tuple(sorted(alleles[g] for g in self.genotype)))


def _pad_left_if_empty(pos: int, ref: str, alts: List[str], genome: str):
    alts = [a.replace("-", "") for a in alts]
    if min(len(x) for x in [ref] + alts) > 0:
        return False, pos, ref, alts
    anchor = genome[pos - 1]
    return True, pos - 1, anchor + ref, [anchor + a for a in alts]


def normalise(pos: int, ref: str, alts: Sequence[str], genome: str):
    """Trim shared suffix bases (re-anchoring on the previous reference base whenever an allele would become
    empty), then shared prefix bases while every allele keeps at least one (vcfFromContigs.py:176-209)."""
    _, pos, ref, alts = _pad_left_if_empty(pos, ref, list(alts), genome)
    if not alts or all(a == ref for a in alts):
        return None
    while True:
        trimmed = len({x[-1] for x in [ref] + alts}) == 1
        if trimmed:
            ref, alts = ref[:-1], [a[:-1] for a in alts]
        padded, pos, ref, alts = _pad_left_if_empty(pos, ref, alts, genome)
        if not (trimmed or padded):
            break
    while len(ref) > 1 and all(len(a) > 1 for a in alts) and len({x[0] for x in [ref] + alts}) == 1:
        pos, ref, alts = pos + 1, ref[1:], [a[1:] for a in alts]
    return pos, ref, alts


def call_site(posteriors: Dict[Tuple[str, str], float], chromosome: str, start: int, length: int,
              genome: str, info: str = "HELLO") -> Optional[Call]:
    """Pair posteriors of one site ({(a, b): p}, values float or 0-dim tensors) -> Call, or None when the
    site holds no non-reference allele."""
    ref_allele = genome[start:start + length]
    best_p, best_pair = max((float(p), pair) for pair, p in posteriors.items())
    qual = -10.0 * math.log10(1.0 - min(best_p, QUAL_CAP))
    alts = sorted(set(best_pair) - {ref_allele})
    if alts:
        genotype = tuple(0 if a == ref_allele else alts.index(a) + 1 for a in best_pair)
    else:
        genotype = (0, 0)
        alts = sorted({a for pair in posteriors for a in pair} - {ref_allele})
        if not alts:
            return None
    norm = normalise(start, ref_allele, alts, genome)
    if norm is None:
        return None
    source = (ref_allele,) + tuple(alts)
    pos, ref, alts = norm
    return Call(chromosome, pos, ref, tuple(alts), genotype, qual, info, source=source)


def mean_posteriors(experts: Sequence[Dict], meta: Sequence[float]) -> Dict:
    """Meta-weighted mean of the three experts' pair posteriors (prepareVcf.py:154-163), in float64."""
    w = [float(m) for m in meta]
    return {pair: sum(float(e[pair]) * wi for e, wi in zip(experts, w)) for pair in experts[0]}


def call_from_prediction(prediction, chromosome: str, start: int, length: int, genome: str) -> Optional[Call]:
    """``prediction`` = what the network returns for a site: a {pair: p} dict, or the 5-tuple
    (mix, e0, e1, e2, meta) -- then the final-VCF rule (mean of experts) is applied."""
    if isinstance(prediction, dict):
        return call_site(prediction, chromosome, start, length, genome)
    _, e0, e1, e2, meta = prediction
    return call_site(mean_posteriors((e0, e1, e2), meta), chromosome, start, length, genome)


# --------------------------------------------------------------------------------------------
# annotations (``--annotate``; the reference writes none: DESIGN.md "Annotations")
# --------------------------------------------------------------------------------------------
ANNOTATED_FORMAT = "GT:GQ:DP:AD:ADF:ADR"
ANNOTATION_HEADER = (
    '##INFO=<ID=MQ,Number=1,Type=Float,Description="Root mean square mapping quality of the reads supporting any allele of the site">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: QUAL rounded, at most 99">\n'
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads supporting any allele of the site">\n'
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads supporting each listed allele">\n'
    '##FORMAT=<ID=ADF,Number=R,Type=Integer,Description="Reads supporting each listed allele on the forward strand">\n'
    '##FORMAT=<ID=ADR,Number=R,Type=Integer,Description="Reads supporting each listed allele on the reverse strand">\n')


def annotate(call: Call, site_alleles: Sequence[str], support0, support1=None) -> str:
    """``call.line()`` with read support: the rules of ``hello_site_records_annotated`` (hello_amd/csrc/records.hip).
    ``support0`` / ``support1``: per allele of the site, in ``site_alleles`` order, the four integers of
    ``hello_engine_allele_support`` (reads, forward reads, sum mapq, sum mapq^2) for each technology; both are summed.

      GQ   min(99, floor(QUAL + 0.5))
      DP   reads over ALL alleles of the site, listed in the record or not
      AD   REF, then each ALT in the record's order: the reads of the site allele whose string equals that allele before
           normalisation (``call.source``), 0 when the site does not hold it; ADF the forward ones, ADR = AD - ADF
      MQ   sqrt(sum mapq^2 / DP) in double, written %.2f; ``.`` when DP is 0
    """
    tables = [[[int(v) for v in row] for row in t] for t in (support0, support1) if t is not None]
    names = list(site_alleles)
    depth = sum(row[0] for t in tables for row in t)
    squares = sum(row[3] for t in tables for row in t)
    ad, adf = [], []
    for allele in call.source:
        a = names.index(allele) if allele in names else None
        ad.append(sum(t[a][0] for t in tables) if a is not None else 0)
        adf.append(sum(t[a][1] for t in tables) if a is not None else 0)
    mq = "%.2f" % math.sqrt(float(squares) / float(depth)) if depth > 0 else "."
    gq = min(99, int(math.floor(call.qual + 0.5)))
    join = lambda values: ",".join(str(v) for v in values)                # noqa: E731
    sample = ":".join(["/".join(str(g) for g in call.genotype), str(gq), str(depth), join(ad), join(adf),
                       join(a - f for a, f in zip(ad, adf))])
    return "%s\t%d\t.\t%s\t%s\t%f\t%s\t%s;MQ=%s\t%s\t%s" % (
        call.chromosome, call.position + 1, call.ref, ",".join(call.alts), call.qual, call.filter, call.info, mq,
        ANNOTATED_FORMAT, sample)


def strip_annotations(line: str) -> str:
    """An annotated record line without its annotations: the line the caller writes without ``--annotate``."""
    cols = line.rstrip("\n").split("\t")
    if len(cols) < 10 or cols[8] != ANNOTATED_FORMAT:
        return line
    cols[7] = cols[7][:cols[7].rindex(";MQ=")]
    cols[8], cols[9] = "GT", cols[9].split(":")[0]
    return "\t".join(cols) + ("\n" if line.endswith("\n") else "")


# --------------------------------------------------------------------------------------------
# genotype likelihoods and base-level evidence (``--annotate_evidence``: DESIGN.md "Evidence")
# --------------------------------------------------------------------------------------------
_EVIDENCE_DECLARATIONS = dict(
    MBQ='##INFO=<ID=MBQ,Number=R,Type=Integer,Description="Mean over the supporting reads of the lowest base quality inside the allele">\n',
    MPOS='##INFO=<ID=MPOS,Number=R,Type=Integer,Description="Mean over the supporting reads of the distance in read bases from the allele to the nearer read end">\n',
    PL='##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods from the pair posteriors, at most 255">\n',
    ADI='##FORMAT=<ID=ADI,Number=R,Type=Integer,Description="Reads supporting each listed allele, first technology (Illumina)">\n',
    ADP='##FORMAT=<ID=ADP,Number=R,Type=Integer,Description="Reads supporting each listed allele, second technology (PacBio)">\n',
    AH1='##FORMAT=<ID=AH1,Number=R,Type=Integer,Description="Reads supporting each listed allele with haplotag 1">\n',
    AH2='##FORMAT=<ID=AH2,Number=R,Type=Integer,Description="Reads supporting each listed allele with haplotag 2">\n')


def evidence_format(two_technologies: bool, hp: bool) -> str:
    """The FORMAT column of an evidence line."""
    return ANNOTATED_FORMAT + ":PL" + (":ADI:ADP" if two_technologies else "") + (":AH1:AH2" if hp else "")


def evidence_header(two_technologies: bool, hp: bool) -> str:
    """The header lines an ``--annotate_evidence`` run adds: those of ``--annotate`` and one per field actually written."""
    keys = ["MBQ", "MPOS", "PL"] + (["ADI", "ADP"] if two_technologies else []) + (["AH1", "AH2"] if hp else [])
    return ANNOTATION_HEADER + "".join(_EVIDENCE_DECLARATIONS[k] for k in keys)


def phred_likelihoods(call: Call, site_alleles: Sequence[str], posteriors: Dict[Tuple[str, str], float]) -> str:
    """``PL`` of a record from the pair posteriors its QUAL comes from: in VCF order (for k: for j <= k) the posterior p_jk of
    the pair of listed alleles {L_j, L_k} (``call.source``), min(255, floor(-10 log10(p_jk / p_max) + 0.5)) with p_max the
    largest of them; 255 for p_jk <= 0; ``.`` when a listed allele is not among the site's alleles or p_max <= 0."""
    names = list(site_alleles)
    if any(allele not in names for allele in call.source):
        return "."
    def value(a, b):
        return float(posteriors[(a, b)] if (a, b) in posteriors else posteriors[(b, a)])
    listed = [value(call.source[j], call.source[k]) for k in range(len(call.source)) for j in range(k + 1)]
    p_max = max(listed)
    if not p_max > 0:
        return "."
    out = []
    for p in listed:
        ratio = p / p_max if p > 0 else 0.0
        out.append(int(min(255.0, math.floor(-10.0 * math.log10(ratio) + 0.5))) if ratio > 0 else 255)
    return ",".join(str(v) for v in out)


def annotate_evidence(call: Call, site_alleles: Sequence[str], posteriors: Dict[Tuple[str, str], float], support0, evidence0,
                      support1=None, evidence1=None, hp: bool = False) -> str:
    """``annotate(call, ...)`` with genotype likelihoods and base-level evidence: the rules of ``hello_site_records_evidence``
    (hello_amd/csrc/records.hip).  ``posteriors``: the {pair: p} the call was made from (``call_site``'s argument).
    ``evidence0`` / ``evidence1``: per allele of the site the six integers of ``hello_engine_allele_evidence`` (reads with a
    base inside the allele nq, sum of their lowest such quality, sum of their distance to the nearer read end, reads with
    haplotag 1, with haplotag 2, guarded reads) for each technology; ``evidence1`` goes with ``support1``.

      PL          ``phred_likelihoods``
      ADI, ADP    AD from technology 0 alone, technology 1 alone (two technologies only)
      AH1, AH2    haplotag 1 / 2 reads per listed allele, both technologies summed (``hp`` only)
      MBQ, MPOS   per listed allele, sums and nq over both technologies: (2 sum + nq) // (2 nq); ``.`` when nq is 0 or the
                  site does not hold the allele
    """
    if (support1 is None) != (evidence1 is None):
        raise ValueError("evidence1 goes with support1")
    base = annotate(call, site_alleles, support0, support1).split("\t")
    support = [[[int(v) for v in row] for row in t] for t in (support0, support1) if t is not None]
    evidence = [[[int(v) for v in row] for row in t] for t in (evidence0, evidence1) if t is not None]
    names = list(site_alleles)
    found = [names.index(allele) if allele in names else None for allele in call.source]
    column = lambda a, k: sum(t[a][k] for t in evidence)                                     # noqa: E731
    join = lambda values: ",".join(str(v) for v in values)                                   # noqa: E731

    def mean(k):
        nq = [column(a, 0) if a is not None else 0 for a in found]
        return join((2 * column(a, k) + n) // (2 * n) if n > 0 else "." for a, n in zip(found, nq))
    two = len(support) == 2
    base[7] += ";MBQ=%s;MPOS=%s" % (mean(1), mean(2))
    base[8] = evidence_format(two, hp)
    sample = [base[9], phred_likelihoods(call, site_alleles, posteriors)]
    if two:
        sample += [join(t[a][0] if a is not None else 0 for a in found) for t in support]
    if hp:
        sample += [join(column(a, k) if a is not None else 0 for a in found) for k in (3, 4)]
    base[9] = ":".join(sample)
    return "\t".join(base)


def strip_evidence(line: str) -> str:
    """An evidence line without PL and the evidence fields: the line ``--annotate`` writes."""
    cols = line.rstrip("\n").split("\t")
    if len(cols) < 10 or not cols[8].startswith(ANNOTATED_FORMAT + ":PL"):
        return line
    cols[7] = cols[7][:cols[7].rindex(";MBQ=")]
    cols[8], cols[9] = ANNOTATED_FORMAT, ":".join(cols[9].split(":")[:ANNOTATED_FORMAT.count(":") + 1])
    return "\t".join(cols) + ("\n" if line.endswith("\n") else "")


# --------------------------------------------------------------------------------------------
# the per-shard ``.features`` records and what prepareVcf makes of them
# --------------------------------------------------------------------------------------------
def feature_record(prediction, chromosome: str, start: int, length: int) -> dict:
    """The dict the per-shard caller appends to its ``.features`` list for one site (reference
    python/caller_calling.py:743-754): chromosome, position (0-based site start), length of the reference
    allele, the meta-expert weights and the three experts' pair posteriors.  ``prediction`` is the network's
    5-tuple (mix, e0, e1, e2, meta).  Values are stored as plain floats / a float32 NumPy array, which is
    what prepareVcf.py:138-163 converts them to anyway, so the reference's own tool reads the file."""
    import numpy as np
    _, e0, e1, e2, meta = prediction
    plain = lambda d: {pair: float(v) for pair, v in d.items()}          # noqa: E731
    meta = np.asarray(meta.detach().cpu().numpy() if hasattr(meta, "detach") else meta, dtype=np.float32)
    return {"chromosome": chromosome, "position": int(start), "length": int(length), "meta": meta,
            "expertPredictions": (plain(e0), plain(e1), plain(e2))}


def write_features(path: str, records: Sequence[dict]) -> str:
    """``<prefix>.features``: one pickled list per shard (caller_calling.py:895-898)."""
    import pickle
    with open(path, "wb") as fh:
        pickle.dump(list(records), fh)
    return path


@dataclass
class ShardCalls:
    """prepareVcf.py:126-176 for one shard: per-expert calls, the call of the expert the meta-expert trusts
    most, the call on the meta-weighted mean (the one the final VCF is built from), and the choices BED rows."""
    expert: Tuple[List[Optional[Call]], List[Optional[Call]], List[Optional[Call]]]
    best: List[Optional[Call]]
    mean: List[Optional[Call]]
    choices: List[Tuple[str, int, int, int]]


def calls_from_features(records: Sequence[dict], genomes: Dict[str, str]) -> ShardCalls:
    """``genomes``: chromosome -> reference sequence (the reference reads it through its ReferenceCache)."""
    expert: Tuple[List, List, List] = ([], [], [])
    best, mean, choices = [], [], []
    for rec in records:
        chrom, pos, length = rec["chromosome"], rec["position"], rec["length"]
        genome = genomes[chrom]
        per_expert = [call_site(p, chrom, pos, length, genome) for p in rec["expertPredictions"]]
        for lst, c in zip(expert, per_expert):
            lst.append(c)
        meta = [float(m) for m in rec["meta"]]
        choice = max(range(3), key=lambda i: (meta[i], -i))              # np.argmax: first maximum
        best.append(per_expert[choice])
        mean.append(call_site(mean_posteriors(rec["expertPredictions"], meta), chrom, pos, length, genome))
        choices.append((chrom, pos, pos + length, choice))
    return ShardCalls(expert, best, mean, choices)
