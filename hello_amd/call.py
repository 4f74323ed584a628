"""Throughput driver with the reference caller's command line.

    python -m hello_amd.call --network model.wrapper.dnn --workdir out --shards 'shards/*.npz' \\
                             [--ref genome.fa] [--num_threads 8] [--include_hp] [--ibam ... --pbam ...]

The reference's ``call.py`` (python/call.py:88-243) detects hotspots, shards them, runs ``caller_calling.main`` per
shard in a process pool -- one site at a time: featurise (C++), score (torch CPU), emit a VCF line, collect the
``.features`` entry (caller_calling.py:859-900) -- checks every shard log for the sentinel ``Completed running the
script`` (:225-229) and lets ``prepareVcf.main`` build the final VCF from the ``.features`` files (:233-241).

This driver keeps that contract.  ``--shards`` starts where a shard's candidate sites exist (``hello_amd.shards``);
``--from_bam`` / ``--from_bams`` start from the BAM(s) and build them on the GPU first (``hello_amd.hotspots``, then
``hello_amd.candidates`` / ``hello_amd.pacbio`` / ``hello_amd.hybrid``; ``hello_amd.route`` says which BAMs, options and
thresholds every stage of a route runs with).  Everything after the candidate sites runs at the engine's rate
(``hello_amd.shard_pipeline``): reader threads load shards with bounded read-ahead; several shards are coalesced into one
GPU launch

    reads + CIGARs --hello_engine_featurize--> uint8 pileups (device) --hello_engine_forward--> logits, meta, pair
    posteriors --hello_site_records (host threads)--> record lines (caller_calling.py:698-743), ``.features`` entries
    (:743-754), final-VCF lines (prepareVcf.py:138-168)

while the previous launch's records are written and the next one's bytes are staged.  Per shard N it writes
``<workdir>/<features dir>/features<N>.vcf``, ``features<N>.features`` (the pickle ``prepareVcf`` reads),
``features<N>.log`` ending in the sentinel and ``features<N>.mean.vcf``; then ``<workdir>/results.output.vcf`` from the
meta-weighted mean of the experts (prepareVcf.py:126-176,199-260; sorted in process instead of by ``vcf-sort``).

``--gpus N`` (or a launch under ``python -m torch.distributed.run``) runs one process per GPU: the shard files are dealt
to the ranks as contiguous runs balanced by read count (``hello_amd.shard.partition_sites`` over per-shard read
totals), every rank writes its shards' files, and after ONE barrier rank 0 merges the final VCF from the files and the
ranks' key indexes -- the ranks exchange no pileup or posterior data (the reference's pool does not either,
call.py:215-221).
The reference's flags for the stages before the candidate sites (--hybrid_hotspot, --q_threshold, --mapq_threshold,
--reconcilement_size) reach those stages with ``--from_bams``; ``--from_bam`` runs them at the defaults, and with ``--shards``
they are accepted so existing command lines keep working.  --ibam / --pbam are the BAM(s) of a BAM route, and always name the
features directory the way ``get_workdir`` does (call.py:40-48).

``--annotate`` (not in the reference, off by default) adds read support to every record line: GQ, DP, AD, ADF, ADR in the sample
column and MQ in INFO, counted on the GPU from the launch's own per-read arrays (``hello_engine_allele_support``); without it
every file is byte for byte what it is with the flag absent.  ``--annotate_evidence`` (implies the fields of ``--annotate``)
adds genotype likelihoods and base-level evidence behind them: PL from the line's own posteriors, MBQ and MPOS in INFO, ADI / ADP
with a two-technology model and AH1 / AH2 with ``--include_hp`` (``hello_engine_allele_evidence``; ``hello_amd.vcf.annotate_evidence``).

``--gvcf`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) writes ``<workdir>/results.output.g.vcf``
after ``results.output.vcf`` is complete: its records byte for byte, and reference-confidence blocks (``<NON_REF>``, ``END``,
``MIN_DP``, ``GQ``, ``PL``) over every other position of the chromosomes called, counted on the GPU in a second pass over the BAM(s)
(``hello_amd.gvcf``).

``--phase`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) writes ``<workdir>/results.output.phased.vcf``
after ``results.output.vcf`` is complete: its lines in its order, the heterozygous records that the reads link rewritten as ``a|b``
with a phase set (``PS``), observed, linked and tagged on the GPU in a pass of its own over the BAM(s) (``hello_amd.phase``;
DESIGN.md section 7g).  ``--phase_fragments`` (with ``--phase`` or ``--haplotag``, off by default) makes the two mates of a read
pair one fragment in that pass: joined by name on the GPU, linked over their merged observations, tagged alike (section 7i).

``--haplotag_vcf V`` (with ``--from_bam`` / ``--from_bams`` and ``--include_hp``, not in the reference, off by default) gives every
read the candidate stage fetches a haplotag from the phased VCF ``V`` (``a|b`` records with ``PS``) in place of the BAM's own ``HP``
tag, on the GPU (``hello_amd.haplotag``) -- the reference's workflow for its haplotagged PacBio model, without
the outside tool that writes a tagged BAM.  ``--haplotag`` needs no phased VCF: pass 1 is this command with ``--phase`` in
``<workdir>/haplotag_pass1``, pass 2 is this command with ``--haplotag_vcf`` on pass 1's ``results.output.phased.vcf``.

``--mark_duplicates`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) finds the PCR duplicates of the
Illumina BAM on the GPU before the hotspot stage (``hello_amd.markdup``) and runs everything after it with flag
0x400 set on them in what ``BamFile.fetch`` returns, so every stage drops them; ``<workdir>/duplicates.metrics.txt`` holds the counts.

``--qc`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) counts alignment, coverage and insert-size
metrics of every BAM of the route on the GPU after ``results.output.vcf`` is complete (``hello_amd.qc``) and
writes ``<workdir>/qc.illumina.*`` and / or ``qc.pacbio.*``: ``metrics.txt``, ``tables.npz``, ``windows.bedgraph`` (``--qc_window``)
and, with ``--qc_regions BED``, ``targets.tsv``.  Under ``--mark_duplicates`` the marked reads count as duplicates and leave the depth.

``--methylation`` (with ``--from_bam --pbam`` / ``--from_bams``, not in the reference, off by default) counts the 5mC calls of the
PacBio BAM's MM / ML tags per CpG site and haplotype on the GPU after ``results.output.vcf`` is complete
(``hello_amd.methylation``) and writes ``<workdir>/methylation.combined.bed``, ``.hap1.bed``, ``.hap2.bed``
and ``methylation.npz``.  A read's haplotype comes from ``--haplotag_vcf``, else from the phased VCF of ``--phase``, else from its HP tag.

``--contamination --contamination_sites V`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) counts the
bases of every BAM of the route at the sites of ``V`` on the GPU after ``results.output.vcf`` is complete
(``hello_amd.contamination``), estimates each BAM's contamination and, with two BAMs, whether they hold one
person, and writes ``<workdir>/contamination.illumina.*`` and / or ``contamination.pacbio.*`` (``txt``, ``pileup.tsv``, ``npz``) and
``contamination.identity.txt``.  Under ``--mark_duplicates`` the marked reads leave the pileup.

``--sv`` (with ``--from_bam`` / ``--from_bams``, not in the reference, off by default) finds the deletions and insertions of at least
``--sv_min_size`` bases that the reads of every BAM of the route carry as one ``D`` or ``I`` operation, on the GPU after
``results.output.vcf`` is complete (``hello_amd.sv``): left-aligned, clustered (``--sv_cluster_gap``,
``--sv_len_ratio``, ``--sv_min_support``) and genotyped against the reads that span them (``--sv_flank``).  It writes
``<workdir>/sv.illumina.*`` and / or ``sv.pacbio.*`` (``vcf`` with symbolic ``<DEL>`` / ``<INS>`` alleles, ``npz``).  With
``--sv_split`` the SA tags of the reads are read too and the junctions of split alignments join the same clusters (``<DUP>`` and
``<INV>`` alleles, the ``SR`` field).  A read's haplotype
comes from ``--haplotag_vcf``, else from the phased VCF of ``--phase``, else from its HP tag; under ``--mark_duplicates`` the marked
reads leave the pass.  With ``--sv_pairs`` the mate fields are read as well: discordant read pairs become rows (``<DEL>``, ``<DUP>``,
``<INV>``; the ``PR`` field), imprecise events are called from pairs alone and the clipped ends near an event are counted (``CE``); the
library's inner distances are sampled from the BAM or given with ``--sv_pairs_library`` (it reads the SA tags
as ``--sv_split`` does).
"""
from __future__ import annotations

import argparse
import glob
import logging
import os
import pickle
import re
import subprocess
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import shards as shard_io
from . import vcf
from .route import Route, chromosome_list, from_bam_route                   # noqa: F401 -- from_bam_route: an entry point here too
from .wrapper import pair_keys

from .shard_pipeline import SENTINEL                 # caller_calling.py:902, checked by call.py:225-229  # noqa: E402
FEATURE_LENGTH = 150                                 # call.py:187


# ------------------------------------------------------------------------------------------------
# reference sequence: a FASTA read as text (no pysam), or the windows the shards carry
# ------------------------------------------------------------------------------------------------
def read_fasta(path: str, wanted: Optional[Sequence[str]] = None) -> Dict[str, str]:
    """chromosome -> sequence (upper / lower case kept).  ``wanted`` limits what is held in memory."""
    keep = set(wanted) if wanted is not None else None
    out: Dict[str, List[str]] = {}
    name = None
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                if keep is not None and name not in keep:
                    name = None
                else:
                    out[name] = []
            elif name is not None:
                out[name].append(line.strip())
    return {k: "".join(v) for k, v in out.items()}


class WindowReference:
    """Genome coordinates served from one site's reference window (what the shard carries when no FASTA is given):
    ``ref[a:b]`` / ``ref[i]`` like a chromosome string."""

    def __init__(self, window: str, window_start: int):
        self.window, self.start = window, window_start

    def __getitem__(self, index):
        if isinstance(index, slice):
            lo, hi = index.start - self.start, index.stop - self.start
            if lo < 0 or hi > len(self.window):
                raise IndexError(f"[{index.start}, {index.stop}) leaves the site's reference window "
                                 f"[{self.start}, {self.start + len(self.window)})")
            return self.window[lo:hi]
        i = index - self.start
        if i < 0 or i >= len(self.window):
            raise IndexError(f"position {index} leaves the site's reference window")
        return self.window[i]


def reference_segment(ref, start: int, stop: int, span: int = FEATURE_LENGTH) -> np.ndarray:
    """caller_calling.py:53-97 (get_reference_segment + one_hot_encode): uint8 [span, 5], ACGT + other."""
    mid = (start + stop) // 2
    left = mid - span // 2
    seg = ref[left:left + span] if left >= 0 else ""
    if len(seg) != span:            # the reference's one_hot_encode yields a short tensor here and the network call fails
        raise ValueError(f"the {span} bp reference segment around [{start}, {stop}) leaves the sequence (it starts at {left})")
    out = np.zeros((span, 5), np.uint8)
    out[np.arange(len(seg)), ["ACGT".find(b) if b in "ACGT" else 4 for b in seg]] = 1
    return out


# ------------------------------------------------------------------------------------------------
# one shard
# ------------------------------------------------------------------------------------------------
def _genome_bytes(genomes: Optional[Dict[str, str]]) -> Optional[Dict[str, bytes]]:
    return {k: (v if isinstance(v, bytes) else v.encode("ascii")) for k, v in genomes.items()} if genomes else None


def score_shard(network, sites, include_hp: bool = False, genomes: Optional[Dict[str, str]] = None,
                feature_length: int = FEATURE_LENGTH, keep=None, annotate: bool = False, evidence: bool = False):
    """Featurise and score every site of ONE shard in one launch, synchronously (the building block under test; the
    driver itself streams shards through ``shard_pipeline.run``).  -> [(record line | None, .features entry | None)] per
    site, in order -- what caller_calling.vcfRecords returns per site (:657-754).  ``sites``: a ``shards.PackedShard``
    or a list of ``shards.CandidateSite``; ``keep``: optional per-site booleans, sites marked False are scored but emit
    nothing; ``annotate``: the record lines carry read support (``hello_amd.vcf.annotate``); ``evidence``: also PL and the
    base-level evidence (``hello_amd.vcf.annotate_evidence``; implies ``annotate``)."""
    from . import records as rec
    from .shard_pipeline import ShardScorer, prepare, site_table
    packed = sites if isinstance(sites, shard_io.PackedShard) else shard_io.PackedShard.from_sites(sites, feature_length)
    if packed.n_sites == 0:
        return []
    scorer = getattr(network, "_shard_scorer", None)
    annotate = bool(annotate) or bool(evidence)
    if scorer is None or scorer.L != feature_length or scorer.annotate != annotate or scorer.evidence != bool(evidence):
        scorer = network._shard_scorer = ShardScorer(network, include_hp, feature_length, annotate=annotate, evidence=evidence)
    elif scorer.channels[0] != (7 if include_hp else 6):
        raise ValueError(f"--include_hp {'set' if include_hp else 'not set'}: the featurizer would write {7 if include_hp else 6} "
                         f"channels, the model reads {scorer.channels[0]}")
    prepare(packed, scorer.hybrid, scorer.uses_ref)
    done = scorer.submit([packed]) + scorer.flush()
    scored = done[-1]
    table = site_table([packed], _genome_bytes(genomes), keep=None if keep is None else np.asarray(keep, np.uint8))
    with rec.site_records(table, scored.posteriors, scored.meta, None, features=True, support=scored.support,
                          evidence=scored.evidence, evidence_fields=scored.evidence_fields) as r:
        entries = iter(pickle.loads(bytes(r.features)))
        out = []
        for s in range(packed.n_sites):
            lo, hi = int(r.shard_vcf_off[s]), int(r.shard_vcf_off[s + 1])
            out.append((bytes(r.shard_vcf[lo:hi - 1]).decode("ascii"), next(entries)) if hi > lo else (None, None))
    return out


def shard_number(path: str, fallback: int) -> int:
    """The N of the reference's ``shard<N>.txt`` / ``features<N>`` (call.py:162-221): the digits that end the file's stem."""
    m = re.search(r"(\d+)$", os.path.splitext(os.path.basename(path))[0])
    return int(m.group(1)) if m else fallback


def natural_key(path: str):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(path))]


# ------------------------------------------------------------------------------------------------
# final VCF (prepareVcf.main)
# ------------------------------------------------------------------------------------------------
def header(chromosomes: Sequence[str], lengths: Dict[str, int], annotate: bool = False, evidence=None) -> str:
    """prepareVcf.py:185-196; ``annotate``: plus the lines that declare MQ, GQ, DP, AD, ADF and ADR; ``evidence``: None, or
    (two technologies, haplotags) of an ``--annotate_evidence`` run -- then ``vcf.evidence_header`` of them instead."""
    s = "##fileformat=VCFv4.1\n"
    for c in chromosomes:
        s += "##contig=<ID=%s,length=%d>\n" % (c, lengths[c]) if c in lengths else "##contig=<ID=%s>\n" % c
    s += '##INFO=<ID=HELLO,Number=1,Type=String,Description="Obtained from HELLO variant caller">\n'
    s += '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    s += '##FILTER=<ID=FAIL,Description="Failed call">\n'
    if evidence is not None:
        s += vcf.evidence_header(*evidence)
    elif annotate:
        s += vcf.ANNOTATION_HEADER
    s += "#" + "\t".join("CHROM  POS     ID      REF     ALT     QUAL    FILTER  INFO    FORMAT  SAMPLE1".split()) + "\n"
    return s


def prepare_vcf(feature_files: Sequence[str], output_path: str, genomes_for, lengths: Dict[str, int]) -> str:
    """prepareVcf.main (:199-260) for the label the pipeline uses ("output" = calls on the meta-weighted mean of
    the experts, :154-168), records sorted by (chromosome, position) in process (the reference pipes through the
    external ``vcf-sort``).  ``genomes_for(chromosome, position)`` -> a sequence addressable in genome coordinates."""
    calls: List[vcf.Call] = []
    chromosomes = []
    for path in feature_files:
        for rec in pickle.load(open(path, "rb")):
            genome = genomes_for(rec)
            mean = vcf.mean_posteriors(rec["expertPredictions"], [float(m) for m in rec["meta"]])
            call = vcf.call_site(mean, rec["chromosome"], rec["position"], rec["length"], genome)
            if call is not None:
                calls.append(call)
            if rec["chromosome"] not in chromosomes:
                chromosomes.append(rec["chromosome"])
    order = {c: i for i, c in enumerate(sorted(chromosomes))}
    calls.sort(key=lambda c: (order[c.chromosome], c.position))
    with open(output_path, "w") as fh:
        fh.write(header(sorted(chromosomes), lengths))
        for c in calls:
            fh.write(c.line() + "\n")
    return output_path


# ------------------------------------------------------------------------------------------------
# command line (python/call.py:245-323)
# ------------------------------------------------------------------------------------------------
def features_dir_name(ibam: Optional[str], pbam: Optional[str]) -> str:
    """call.py:33-48 (get_bam_string / get_workdir)."""
    def bam_string(bam):
        bam = os.path.abspath(bam)
        name = os.path.split(os.path.split(bam)[0])[-1].replace("/", "__") + "___" + os.path.split(bam)[-1].replace("/", "__")
        return name.replace(".", "__")
    name = "features"
    for bam in (ibam, pbam):
        if bam:
            name += "_" + bam_string(bam)
    return name


def parser() -> argparse.ArgumentParser:
    from . import sv
    ap = argparse.ArgumentParser(description="HELLO variant scoring on MI355X, with call.py's command line")
    ap.add_argument("--ibam", help="Illumina BAM file (names the features directory; read by --from_bam / --from_bams)")
    ap.add_argument("--pbam", help="PacBio BAM file (names the features directory; read by --from_bam / --from_bams)")
    ap.add_argument("--ref", help="Reference FASTA (optional when the shards carry their reference windows)")
    ap.add_argument("--workdir", required=True, help="Working directory")
    ap.add_argument("--chromosomes", help="Chromosomes to use (comma-separated): shards' sites elsewhere are skipped")
    ap.add_argument("--network", required=True, help="Network path (.wrapper.dnn pickle or native .npz)")
    ap.add_argument("--hybrid_hotspot", default=False, action="store_true", help="(upstream stage; accepted)")
    ap.add_argument("--q_threshold", default=10, type=int, help="(upstream stage; accepted)")
    ap.add_argument("--mapq_threshold", default=10, type=int, help="(upstream stage; accepted)")
    ap.add_argument("--num_threads", type=int, default=30,
                    help="host threads per GPU: shard readers and the record stage share them (the reference's pool size)")
    ap.add_argument("--reconcilement_size", default=10, type=int, help="(upstream stage; accepted)")
    ap.add_argument("--include_hp", default=False, action="store_true", help="Include HP tags in tensors")
    ap.add_argument("--shards", required=False,
                    help="glob (or directory) of pre-extracted candidate-site shards (hello_amd.shards), one per "
                         "reference shard<N>.txt")
    ap.add_argument("--from_bam", action="store_true", default=False,
                    help="start from --ibam (or --pbam) and --ref: hotspots, sharding and candidate sites run on the GPU "
                         "(hello_amd.hotspots, hello_amd.candidates / hello_amd.pacbio) and the shards they write under --workdir are "
                         "scored; one Illumina BAM or one PacBio BAM")
    ap.add_argument("--from_bams", action="store_true", default=False,
                    help="start from --ibam AND --pbam and --ref: hotspots over both BAMs (honouring --hybrid_hotspot), sharding and "
                         "hybrid candidate sites (--reconcilement_size) run on the GPU (hello_amd.hotspots, hello_amd.hybrid) and the "
                         "two-technology shards they write under --workdir are scored; --network is a two-technology model")
    ap.add_argument("--resident", action="store_true", default=False,
                    help="with --from_bam / --from_bams: the candidate sites stay on the GPU and are scored in this process as they "
                         "are built -- no <workdir>/shards, no read written to disk; the VCF is the same (one GPU)")
    ap.add_argument("--annotate", action="store_true", default=False,
                    help="write read support into every record: GQ, DP, AD, ADF, ADR in the sample column and MQ in INFO, counted on "
                         "the GPU from the reads each launch scores (not in the reference; off: the files are the reference's)")
    ap.add_argument("--annotate_evidence", action="store_true", default=False,
                    help="the fields of --annotate plus PL from the record's own posteriors, mean base quality (MBQ) and read "
                         "position (MPOS) per allele in INFO, ADI / ADP (depth per technology) with a two-technology model and "
                         "AH1 / AH2 (depth per haplotag) with --include_hp, from the reads each launch scores (not in the reference)")
    ap.add_argument("--gvcf", action="store_true", default=False,
                    help="with --from_bam / --from_bams: also write <workdir>/results.output.g.vcf -- the records of results.output.vcf "
                         "plus reference-confidence blocks (<NON_REF>, END, MIN_DP, GQ, PL) over every other position, counted on "
                         "the GPU in a second pass over the BAM(s) (not in the reference; one GPU)")
    ap.add_argument("--gvcf_gq_binsize", type=int, default=5,
                    help="--gvcf: consecutive positions whose GQ falls into one band of this width share a block (at least 1)")
    ap.add_argument("--phase", action="store_true", default=False,
                    help="with --from_bam / --from_bams: also write <workdir>/results.output.phased.vcf -- the lines of "
                         "results.output.vcf, heterozygous records that the reads link rewritten as a|b with a phase set (PS), "
                         "from a pass of its own over the BAM(s) on the GPU (not in the reference; one GPU)")
    ap.add_argument("--phase_window", type=int, default=8,
                    help="--phase: a record is linked to this many heterozygous records before it (1 to 32)")
    ap.add_argument("--phase_min_margin", type=int, default=2,
                    help="--phase: the smallest |cis - trans| read count that joins a record to a phase set (at least 1)")
    ap.add_argument("--phase_fragments", action="store_true", default=False,
                    help="--phase / --haplotag: the two mates of a read pair act as one fragment -- joined by name on the GPU, "
                         "linked over their merged observations and given one haplotag (not in the reference; DESIGN.md 7i)")
    ap.add_argument("--haplotag_vcf",
                    help="with --from_bam / --from_bams and --include_hp: a phased VCF (a|b records with PS); every read the candidate "
                         "stage fetches gets its haplotag from it on the GPU, in place of the BAM's own HP tag (not in the reference; "
                         "one GPU)")
    ap.add_argument("--haplotag", action="store_true", default=False,
                    help="with --from_bam / --from_bams and --include_hp: two passes -- this command with --phase in "
                         "<workdir>/haplotag_pass1, then this command with --haplotag_vcf on the phased VCF of pass 1 (not in the "
                         "reference; one GPU)")
    ap.add_argument("--mark_duplicates", action="store_true", default=False,
                    help="with --from_bam / --from_bams: find the PCR duplicates of the Illumina BAM on the GPU first and let every "
                         "stage drop them, as if the BAM carried flag 0x400 on them; writes <workdir>/duplicates.metrics.txt (not in "
                         "the reference; one GPU; DESIGN.md 7j)")
    ap.add_argument("--qc", action="store_true", default=False,
                    help="with --from_bam / --from_bams: count flag, mapping-quality, length, per-cycle quality and mismatch, depth "
                         "and insert-size tables of every BAM of the route on the GPU and write <workdir>/qc.illumina.* / "
                         "qc.pacbio.* (metrics.txt, tables.npz, windows.bedgraph; not in the reference; one GPU; DESIGN.md 7k)")
    ap.add_argument("--qc_regions", help="--qc: a BED file of target intervals; depth on target and per target (targets.tsv)")
    ap.add_argument("--qc_window", type=int, default=None, help="--qc: width of the depth windows of windows.bedgraph (default 1000)")
    ap.add_argument("--methylation", action="store_true", default=False,
                    help="with --from_bam --pbam / --from_bams: count the 5mC calls of the PacBio BAM's MM / ML tags per CpG site and "
                         "haplotype on the GPU and write <workdir>/methylation.{combined,hap1,hap2}.bed and methylation.npz; the "
                         "haplotypes come from --haplotag_vcf, else --phase, else the HP tags (not in the reference; one GPU; "
                         "DESIGN.md 7m)")
    ap.add_argument("--contamination", action="store_true", default=False,
                    help="with --from_bam / --from_bams and --contamination_sites: count the bases of every BAM of the route at the "
                         "sites on the GPU, estimate its contamination and, with two BAMs, whether they hold one person; writes "
                         "<workdir>/contamination.illumina.* / contamination.pacbio.* (txt, pileup.tsv, npz) and "
                         "contamination.identity.txt (not in the reference; one GPU; DESIGN.md 7n)")
    ap.add_argument("--contamination_sites", help="--contamination: a VCF (plain or .gz) of biallelic SNVs with INFO AF, common ones")
    ap.add_argument("--sv", action="store_true", default=False,
                    help="with --from_bam / --from_bams: find the deletions and insertions of at least --sv_min_size bases that the "
                         "reads of every BAM of the route carry as one D or I operation, on the GPU, and write <workdir>/sv.illumina.* "
                         "/ sv.pacbio.* (vcf, npz); the haplotypes come from --haplotag_vcf, else --phase, else the HP tags (not in "
                         "the reference; one GPU; DESIGN.md 7p)")
    sv.add_options(ap, given_or_none=True)
    ap.add_argument("--sv_pairs", action="store_true", default=False,
                    help="with --sv: also read the mate fields (and the SA tags) of the reads and call deletions, duplications, inversions "
                         "and translocation ends from discordant read pairs; sv.*.vcf gains the PR, CE, IMPRECISE and CIEND fields (not "
                         "in the reference; DESIGN.md section 7s)")
    sv.add_pairs_options(ap, "sv_", given_or_none=True)
    ap.add_argument("--sv_split", action="store_true", default=False,
                    help="with --sv: also read the SA tags of the reads and call deletions, insertions, duplications and inversions "
                         "from split alignments; sv.*.vcf gains <DUP> and <INV> alleles and the SR field (not in the reference; "
                         "DESIGN.md section 7q)")
    ap.add_argument("--device", type=int, default=0, help="GPU of a single-process run")
    ap.add_argument("--gpus", type=int, default=1,
                    help="processes / GPUs of this node: > 1 re-launches this command under torch.distributed.run "
                         "(a launch that is already under it reads RANK / WORLD_SIZE instead)")
    ap.add_argument("--sites_per_launch", type=int, default=8192, help="shards are coalesced into GPU launches of about this many sites")
    ap.add_argument("--arithmetic", choices=["fp32", "bf16x3", "bf16x3+32"], default="fp32",
                    help="fp32: exact fp32 everywhere (default).  bf16x3: the read convolver's 64-channel trunk on the bf16 matrix "
                         "cores as 3-term splits (~1.3x faster; posteriors move by ~1e-6)")
    return ap


def _header_evidence(args, network):
    """``header``'s ``evidence`` argument: None without --annotate_evidence, else (two-technology model, --include_hp)."""
    if not getattr(args, "annotate_evidence", False):
        return None
    return bool(network.engine.program.channels1), bool(args.include_hp)


def _argv_of(args) -> List[str]:
    argv: List[str] = []
    for action in parser()._actions:
        if not action.option_strings or action.dest in ("help", "gpus"):
            continue
        value = getattr(args, action.dest, None)
        if value is None or value is False:
            continue
        argv += [action.option_strings[0]] + ([] if value is True else [str(value)])
    return argv


def _launch_ranks(args) -> int:
    """``--gpus N`` from a plain command line: one child process per GPU under torch.distributed.run, started BEFORE this
    process touches the GPU; this process only waits for them."""
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "hello_amd.call"] + _argv_of(args) + ["--gpus", str(args.gpus)]
    return subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))).returncode


def _resident_mb() -> float:
    try:
        with open("/proc/self/statm") as fh:
            return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 1e6
    except (OSError, ValueError, IndexError):
        return float("nan")


def shard_read_totals(paths: Sequence[str], threads: int = 4) -> np.ndarray:
    """Reads the featurizer will write per shard (both technologies; dummy reads included): the weight shards are dealt
    to ranks by.  Only the count arrays of each file are read."""
    from concurrent.futures import ThreadPoolExecutor

    def total(path):
        # the second technology's counts weigh in only when the shard says it has one (has_second; a file that carries
        # reads_per_allele1 with has_second = 0 is refused later by PackedShard.validate -- it must not skew the deal first)
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                got = {k: z[k] for k in ("reads_per_allele0", "reads_per_allele1", "has_second") if k in z.files}
        else:
            got = shard_io.read_flat_arrays(path, ("reads_per_allele0", "reads_per_allele1", "has_second"))
        second = "has_second" in got and int(np.asarray(got["has_second"]).reshape(-1)[0]) != 0
        return sum(int(np.maximum(got[k], 1).sum()) for k in (("reads_per_allele0", "reads_per_allele1") if second else ("reads_per_allele0",))
                   if k in got)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        return np.array(list(pool.map(total, paths)), np.int64)


def _shard_files(ns):
    """The hotspot stage per chromosome (``hotspots.txt`` in the reference's ``hotspots_<chrom>_<bam>`` directory), then
    ``shard<N>.txt`` beside it (shardHotspots): yields (N, the shard file) as each is written."""
    from . import candidates as cd, hotspots as hs
    n = 0
    for hotspot_name in hs.run_workdir(ns):
        for chrom, pos in cd.read_positions(hotspot_name).items():
            for part in cd.shard_positions(pos):
                name = os.path.join(os.path.dirname(hotspot_name), "shard%d.txt" % n)
                hs.write_positions(name, chrom, part)
                yield n, name
                n += 1
    if n == 0:
        raise SystemExit("no hotspot was found: nothing to call")


def _shards_of(args, two_bams: bool) -> str:
    """python/call.py:111-221 up to the per-shard caller, on the GPU, for the route of ``args`` (``hello_amd.route``): per
    chromosome hotspots.txt in the reference's ``hotspots_<chrom>_<bam(s)>`` directory, ``shard<N>.txt`` files beside it
    (shardHotspots) and one ``shard<N>.hshard`` per shard file in ``<workdir>/shards``.  Returns that directory."""
    from . import candidates as cd
    logger = logging.getLogger("hello_amd.call")
    route = Route.from_args(args, two_bams)
    genome = read_fasta(route.ref, route.chromosomes)
    tagger = haplotagger_of(args, route)
    find, kw = route.finder(tagger)
    out_dir = os.path.join(args.workdir, "shards")
    os.makedirs(out_dir, exist_ok=True)
    for n, name in _shard_files(route.hotspot_args(args.workdir, genome)):
        _, st = cd.run_activity(list(route.bams), route.ref, name, os.path.join(out_dir, "shard%d" % n), genome=genome, find=find, **kw)
        if two_bams:
            logger.info("%s: %d sites, %d PacBio reads reassigned", name, st.get("sites", 0), st.get("pacbio_reads_reassigned", 0))
        else:
            logger.info("%s: %d sites", name, st.get("sites", 0))
    _close_haplotagger(tagger)
    return out_dir


def shards_from_bam(args) -> str:
    """``<workdir>/shards`` of --from_bam: one Illumina BAM or one PacBio BAM, every stage at the default thresholds."""
    return _shards_of(args, False)


def shards_from_bams(args) -> str:
    """``<workdir>/shards`` of --from_bams, the hybrid caller (python/call.py:111-221 with both BAMs): two-technology shards
    (hello_amd.hybrid), every stage with ``--hybrid_hotspot``, ``--reconcilement_size`` and the two thresholds of the command line."""
    return _shards_of(args, True)


def _bam_route(args) -> bool:
    """A BAM route is selected: --from_bam or --from_bams."""
    return bool(getattr(args, "from_bam", False) or getattr(args, "from_bams", False))


def _under_launcher() -> bool:
    return "RANK" in os.environ and "WORLD_SIZE" in os.environ


def _several_processes(args) -> bool:
    """Not one process on one GPU: --gpus above 1, or a launch under torch.distributed.run."""
    return getattr(args, "gpus", 1) > 1 or _under_launcher()


def check_resident(args) -> None:
    """The refusals of --resident, each naming the fix."""
    if not getattr(args, "resident", False):
        return
    if not _bam_route(args):
        raise SystemExit("--resident keeps the candidate sites of --from_bam / --from_bams on the GPU: add --from_bam (one BAM) or "
                         "--from_bams (--ibam and --pbam), or drop --resident")
    if getattr(args, "from_bam", False) and getattr(args, "from_bams", False):
        raise SystemExit("--from_bam (one BAM) and --from_bams (an Illumina and a PacBio BAM) exclude each other")
    if args.shards:
        raise SystemExit("--resident builds its candidate sites itself and reads no shard files: drop --shards, or drop --resident to "
                         "score the shard files")
    if _several_processes(args):
        raise SystemExit("--resident builds candidate sites on one GPU in one process: run it with --gpus 1 as a plain command, or drop "
                         "--resident (the shard files of --from_bam / --from_bams can be dealt to several GPUs)")


def check_gvcf(args) -> None:
    """The refusals of --gvcf, each naming the fix."""
    if not getattr(args, "gvcf", False):
        return
    if not _bam_route(args):
        raise SystemExit("--gvcf counts the reads of the BAM(s) between the records, and the shard route has no BAM on its path: add "
                         "--from_bam (one BAM) or --from_bams (--ibam and --pbam), or drop --gvcf (python -m hello_amd.gvcf writes a "
                         "gVCF from a VCF that exists and its BAMs)")
    if _several_processes(args):
        raise SystemExit("--gvcf runs its pass over the BAM(s) in one process on one GPU: run it with --gpus 1 as a plain command, or "
                         "drop --gvcf and run python -m hello_amd.gvcf on the finished results.output.vcf")
    if getattr(args, "gvcf_gq_binsize", 5) < 1:
        raise SystemExit("--gvcf_gq_binsize is the width of a GQ band: give 1 or more")


def gvcf_pass(args, result_path: str, genome: Dict[str, str]) -> Optional[str]:
    """--gvcf: ``results.output.g.vcf`` beside the finished ``result_path``, at the thresholds the route's own stages ran with."""
    if not getattr(args, "gvcf", False):
        return None
    from . import gvcf
    route = Route.from_args(args, need_ref=False)
    out = result_path[:-len(".vcf")] + ".g.vcf"
    t0 = time.perf_counter()
    stats: dict = {}
    gvcf.write_gvcf(result_path, list(route.bams), genome, out, route.chromosomes or list(genome), route.q_threshold,
                    route.mapq_threshold, args.gvcf_gq_binsize, route.device, stats=stats)
    logging.getLogger("hello_amd.call").info(
        "gVCF pass: %d blocks in %s, %.2f s (BAM decode %.2f s, kernels %.1f ms)", int(stats.get("blocks", 0)), out,
        time.perf_counter() - t0, stats.get("decode_s", 0.0), stats.get("kernel_ms", 0.0))
    return out


def check_phase(args) -> None:
    """The refusals of --phase and --phase_fragments, each naming the fix."""
    if getattr(args, "phase_fragments", False) and not (getattr(args, "phase", False) or getattr(args, "haplotag", False)):
        raise SystemExit("--phase_fragments is a mode of the phasing pass and there is none in this run: add --phase (a phased VCF "
                         "beside the result) or --haplotag (its pass 1 phases), or drop --phase_fragments")
    if not getattr(args, "phase", False):
        return
    if not _bam_route(args):
        raise SystemExit("--phase reads the alleles of neighbouring records off the reads of the BAM(s), and the shard route has no BAM "
                         "on its path: add --from_bam (one BAM) or --from_bams (--ibam and --pbam), or drop --phase (python -m "
                         "hello_amd.phase phases a VCF that exists from its BAMs)")
    if _several_processes(args):
        raise SystemExit("--phase runs its pass over the BAM(s) in one process on one GPU: run it with --gpus 1 as a plain command, or "
                         "drop --phase and run python -m hello_amd.phase on the finished results.output.vcf")
    if not 1 <= getattr(args, "phase_window", 8) <= 32:
        raise SystemExit("--phase_window is the number of records a record is linked back to: give 1 to 32")
    if getattr(args, "phase_min_margin", 2) < 1:
        raise SystemExit("--phase_min_margin is the smallest |cis - trans| that joins a phase set: give 1 or more")


def phase_pass(args, result_path: str) -> Optional[str]:
    """--phase: ``results.output.phased.vcf`` beside the finished ``result_path``, at the thresholds the route's own stages ran with."""
    if not getattr(args, "phase", False):
        return None
    from . import phase
    route = Route.from_args(args, need_ref=False)
    out = result_path[:-len(".vcf")] + ".phased.vcf"
    t0 = time.perf_counter()
    stats: dict = {}
    fragments = bool(getattr(args, "phase_fragments", False))
    phase.write_phased_vcf(result_path, list(route.bams), out, route.chromosomes, route.q_threshold,
                           route.mapq_threshold, args.phase_window, args.phase_min_margin, route.device, stats=stats,
                           **({"fragments": True} if fragments else {}))           # without the flag: the call of 7g, as it was
    logging.getLogger("hello_amd.call").info(
        "phase pass: %d slots of %d reads in %s, %.2f s (BAM decode %.2f s, kernels %.1f ms)", int(stats.get("slots", 0)),
        int(stats.get("reads_counted", 0)), out, time.perf_counter() - t0, stats.get("decode_s", 0.0),
        sum(stats.get(k, 0.0) for k in ("observe_ms", "link_ms", "tag_ms", "pair_ms", "fragment_link_ms", "fragment_tag_ms")))
    if fragments:
        logging.getLogger("hello_amd.call").info("--phase_fragments: %d pairs joined, %d groups of reads with one name left apart",
                                                 int(stats.get("pairs", 0)), int(stats.get("groups_refused", 0)))
    return out


def check_haplotag(args) -> None:
    """The refusals of --haplotag_vcf and --haplotag, each naming the fix."""
    vcf_given, two_passes = bool(getattr(args, "haplotag_vcf", None)), bool(getattr(args, "haplotag", False))
    if not (vcf_given or two_passes):
        return
    flag = "--haplotag_vcf" if vcf_given else "--haplotag"
    if vcf_given and two_passes:
        raise SystemExit("--haplotag_vcf tags the reads from a phased VCF that exists, --haplotag from one it makes in a first pass: "
                         "give one of the two")
    if not _bam_route(args) or args.shards:
        raise SystemExit(f"{flag} tags the reads the candidate stage fetches from the BAM(s), and shard files hold reads that were "
                         f"fetched before: add --from_bam (one BAM) or --from_bams (--ibam and --pbam) and drop --shards, or drop {flag}")
    if not getattr(args, "include_hp", False):
        raise SystemExit(f"{flag} without --include_hp: the model would not read the haplotags (six pileup channels); add --include_hp "
                         f"with a model of seven channels, or drop {flag}")
    if _several_processes(args):
        raise SystemExit(f"{flag} tags the reads in the process that builds the candidate sites, on one GPU: run it with --gpus 1 as a "
                         f"plain command, or drop {flag}")


def haplotagger_of(args, route: Optional[Route] = None):
    """--haplotag_vcf: one ``haplotag.Haplotagger`` over the file, at the thresholds of ``route`` (default: the route of ``args``);
    None without the flag."""
    if not getattr(args, "haplotag_vcf", None):
        return None
    from . import haplotag
    route = route or Route.from_args(args, need_ref=False)
    return haplotag.Haplotagger(args.haplotag_vcf, route.chromosomes, route.q_threshold, route.mapq_threshold, route.device)


def _close_haplotagger(tagger) -> None:
    if tagger is None:
        return
    st = tagger.stats
    tagger.close()
    logging.getLogger("hello_amd.call").info(
        "haplotags from %d phased records: %d reads tagged 1, %d tagged 2, %d tagged 0 in %d calls (kernel %.1f ms of %.1f ms)",
        int(st["records"]), int(st["reads_hp1"]), int(st["reads_hp2"]), int(st["reads"] - st["reads_hp1"] - st["reads_hp2"]),
        int(st["calls"]), st["kernel_ms"], st["total_ms"])


def haplotag_passes(args) -> str:
    """--haplotag: pass 1 is this command without --haplotag, --gvcf, --qc, --annotate and --annotate_evidence and with --phase, in
    ``<workdir>/haplotag_pass1``; pass 2 is this command with --haplotag_vcf on pass 1's phased VCF, in ``<workdir>``.  Both run in
    this process, each as the command would run alone (the hotspot stage runs twice).  --phase_fragments goes to pass 1, and to
    pass 2 only where --phase was given as well."""
    logger = logging.getLogger("hello_amd.call")
    first = argparse.Namespace(**vars(args))
    first.haplotag = first.gvcf = first.annotate = first.annotate_evidence = first.qc = first.methylation = False
    first.contamination = first.sv = first.sv_split = first.sv_pairs = False
    first.sv_pairs_library = first.sv_pairs_k = first.sv_clip_min = None
    first.qc_regions = first.qc_window = first.contamination_sites = None
    for flag in SV_OPTIONS:
        setattr(first, flag, None)
    first.phase = True
    first.workdir = os.path.join(args.workdir, "haplotag_pass1")
    phased_path = main(first)[:-len(".vcf")] + ".phased.vcf"
    logger.info("--haplotag: pass 1 wrote %s; pass 2 tags the reads from it", phased_path)
    second = argparse.Namespace(**vars(args))
    second.haplotag = False
    second.phase_fragments = bool(getattr(args, "phase_fragments", False) and getattr(args, "phase", False))   # else pass 1's alone
    second.haplotag_vcf = phased_path
    return main(second)


def check_mark_duplicates(args) -> None:
    """The refusals of --mark_duplicates, each naming the fix."""
    if not getattr(args, "mark_duplicates", False):
        return
    if args.shards:
        raise SystemExit("--mark_duplicates marks the reads the stages fetch from the BAM, and shard files hold reads that were fetched "
                         "before: drop --shards and start from the BAM with --from_bam or --from_bams, or drop --mark_duplicates")
    if not _bam_route(args):
        raise SystemExit("--mark_duplicates finds the duplicates among the reads of the Illumina BAM, and this run has no BAM on its "
                         "path: add --from_bam (one BAM) or --from_bams (--ibam and --pbam), or drop --mark_duplicates (python -m "
                         "hello_amd.markdup saves the marks of a BAM on its own)")
    if _several_processes(args):
        raise SystemExit("--mark_duplicates hands its marks to the stages of its own process, on one GPU: run it with --gpus 1 as a "
                         "plain command, or drop --mark_duplicates")
    if not args.ibam:
        raise SystemExit("--mark_duplicates keys a read pair by the 5' ends of both mates, which PacBio reads do not have, and the "
                         "only BAM of this run is --pbam: give the Illumina BAM as --ibam, or drop --mark_duplicates")


def with_duplicates_marked(args) -> str:
    """--mark_duplicates: the marks of the route's Illumina BAM, once, then this command without the flag inside
    ``markdup.applied`` -- every fetch of every stage (both passes of --haplotag too) sees flag 0x400 on the duplicates.  With
    --from_bams the PacBio BAM is left as it is."""
    from . import markdup
    logger = logging.getLogger("hello_amd.call")
    route = Route.from_args(args, need_ref=False)
    os.makedirs(args.workdir, exist_ok=True)
    stats: dict = {}
    marks = markdup.find_duplicates(route.bams[0], route.chromosomes, device=route.device, stats=stats)
    marks.write_metrics(os.path.join(args.workdir, "duplicates.metrics.txt"))
    total = marks.total()
    logger.info("--mark_duplicates: %d reads, %d pairs, %d duplicate reads (%d pairs, %d singles) in %.2f s (BAM decode %.2f s, "
                "kernels %.1f ms)", total["reads"], total["pairs"], total["duplicate_reads"], total["duplicate_pairs"],
                total["duplicate_singles"], stats.get("total_s", 0.0), stats.get("decode_s", 0.0),
                sum(stats.get(k, 0.0) for k in ("ends_ms", "pair_ms", "key_ms", "mark_ms")))
    rest = argparse.Namespace(**vars(args))
    rest.mark_duplicates = False
    with markdup.applied({route.bams[0]: marks}):
        return main(rest)


def check_qc(args) -> None:
    """The refusals of --qc, --qc_regions and --qc_window, each naming the fix."""
    if not getattr(args, "qc", False):
        for flag in ("qc_regions", "qc_window"):
            if getattr(args, flag, None) is not None:
                raise SystemExit(f"--{flag} is an option of the metrics pass and there is none in this run: add --qc, or drop --{flag}")
        return
    if args.shards:
        raise SystemExit("--qc measures the reads of the BAM(s), and shard files hold reads that were fetched and filtered before: "
                         "drop --shards and start from the BAM with --from_bam or --from_bams, or drop --qc")
    if not _bam_route(args):
        raise SystemExit("--qc measures the reads of the BAM(s), and this run has no BAM on its path: add --from_bam (one BAM) or "
                         "--from_bams (--ibam and --pbam), or drop --qc (python -m hello_amd.qc measures a BAM on its own)")
    if _several_processes(args):
        raise SystemExit("--qc runs its pass over the BAM(s) in one process on one GPU: run it with --gpus 1 as a plain command, or "
                         "drop --qc and run python -m hello_amd.qc on the BAM(s)")
    if getattr(args, "qc_window", None) is not None and args.qc_window < 1:
        raise SystemExit("--qc_window is the width of a depth window: give 1 or more")


def qc_pass(args, genome: Dict[str, str]) -> List[str]:
    """--qc: the metrics of every BAM of the route, at the route's --mapq_threshold and chromosomes -> the files written,
    ``<workdir>/qc.illumina.*`` and / or ``qc.pacbio.*``."""
    if not getattr(args, "qc", False):
        return []
    from . import qc
    route = Route.from_args(args, need_ref=False)
    names = ("pacbio",) if route.pacbio else ("illumina", "pacbio")
    targets = qc.read_bed(args.qc_regions) if getattr(args, "qc_regions", None) else None
    window = qc.DEFAULT_WINDOW if getattr(args, "qc_window", None) is None else args.qc_window
    written: List[str] = []
    for bam, name in zip(route.bams, names):
        stats: dict = {}
        metrics = qc.measure(bam, genome, route.chromosomes or list(genome), targets, window, route.mapq_threshold,
                             device=route.device, stats=stats)
        written += metrics.write_all(os.path.join(args.workdir, "qc." + name))
        total = metrics.total()
        logging.getLogger("hello_amd.call").info(
            "--qc %s: %d reads, %d measured, %d pairs in %.2f s (BAM decode %.2f s, kernels %.1f ms)", name, int(total["FLAGS"][0]),
            int(total["STATS"][0]), int(total["STATS"][4]), stats.get("total_s", 0.0), stats.get("decode_s", 0.0),
            sum(stats.get(k, 0.0) for k in ("reads_ms", "depth_ms", "pair_ms", "insert_ms")))
    return written


def check_methylation(args) -> None:
    """The refusals of --methylation, each naming the fix."""
    if not getattr(args, "methylation", False):
        return
    if args.shards:
        raise SystemExit("--methylation reads the MM / ML tags of the PacBio BAM, and shard files hold reads that were fetched before "
                         "without them: drop --shards and start from the BAM with --from_bam or --from_bams, or drop --methylation")
    if not _bam_route(args):
        raise SystemExit("--methylation reads the MM / ML tags of the PacBio BAM, and this run has no BAM on its path: add --from_bam "
                         "(with --pbam) or --from_bams (--ibam and --pbam), or drop --methylation (python -m hello_amd.methylation "
                         "counts a BAM on its own)")
    if _several_processes(args):
        raise SystemExit("--methylation runs its pass over the BAM in one process on one GPU: run it with --gpus 1 as a plain command, "
                         "or drop --methylation and run python -m hello_amd.methylation on the BAM")
    if not args.pbam:
        raise SystemExit("--methylation counts the 5mC calls a PacBio instrument writes into MM / ML, and this route has no PacBio "
                         "BAM: give it as --pbam, or drop --methylation")


def methylation_pass(args, genome: Dict[str, str], result_path: str) -> List[str]:
    """--methylation: the CpG methylation of the route's PacBio BAM at the route's --mapq_threshold and chromosomes -> the files
    written, ``<workdir>/methylation.*.bed`` and ``methylation.npz``.  The reads' haplotypes: --haplotag_vcf, else the phased VCF
    --phase wrote beside ``result_path``, else the BAM's HP tags."""
    if not getattr(args, "methylation", False):
        return []
    from . import haplotag, methylation
    route = Route.from_args(args, need_ref=False)
    phased = getattr(args, "haplotag_vcf", None) or (result_path[:-len(".vcf")] + ".phased.vcf" if getattr(args, "phase", False) else None)
    tagger = haplotag.Haplotagger(phased, route.chromosomes, route.q_threshold, route.mapq_threshold, route.device) if phased else None
    stats: dict = {}
    try:
        found = methylation.measure(route.bams[-1], genome, route.chromosomes or list(genome), tagger, route.mapq_threshold,
                                    device=route.device, stats=stats)
    finally:
        if tagger is not None:
            tagger.close()
    prefix = os.path.join(args.workdir, "methylation")
    written = found.write_bed(prefix) + [found.save(prefix + ".npz")]
    total = found.total()
    logging.getLogger("hello_amd.call").info(
        "--methylation: %d sites, %d reads counting (%d without calls, %d bad, %d hard-clipped), %d observations in %.2f s (BAM decode "
        "%.2f s, kernels %.1f ms; haplotypes from %s)", total["n_sites"], total["counting"], total["reads_no_mods"],
        total["reads_bad_mods"], total["reads_hard_clipped"], total["observations"], stats.get("total_s", 0.0),
        stats.get("decode_s", 0.0), stats.get("sites_ms", 0.0) + stats.get("reads_ms", 0.0), phased or "the HP tags")
    return written


def check_contamination(args) -> None:
    """The refusals of --contamination and --contamination_sites, each naming the fix."""
    if not getattr(args, "contamination", False):
        if getattr(args, "contamination_sites", None) is not None:
            raise SystemExit("--contamination_sites is an option of the contamination pass and there is none in this run: add "
                             "--contamination, or drop --contamination_sites")
        return
    if getattr(args, "contamination_sites", None) is None:
        raise SystemExit("--contamination counts the reads at known sites and was given none: add --contamination_sites with a VCF "
                         "of common biallelic SNVs that carry INFO AF, or drop --contamination")
    if args.shards:
        raise SystemExit("--contamination counts the reads of the BAM(s), and shard files hold reads that were fetched and filtered "
                         "before: drop --shards and start from the BAM with --from_bam or --from_bams, or drop --contamination")
    if not _bam_route(args):
        raise SystemExit("--contamination counts the reads of the BAM(s), and this run has no BAM on its path: add --from_bam (one "
                         "BAM) or --from_bams (--ibam and --pbam), or drop --contamination (python -m hello_amd.contamination "
                         "measures BAMs on their own)")
    if _several_processes(args):
        raise SystemExit("--contamination runs its pass over the BAM(s) in one process on one GPU: run it with --gpus 1 as a plain "
                         "command, or drop --contamination and run python -m hello_amd.contamination on the BAM(s)")


def contamination_pass(args, genome: Dict[str, str]) -> List[str]:
    """--contamination: the pileup at --contamination_sites of every BAM of the route, at the route's thresholds and chromosomes,
    and the estimates on it -> the files written, ``<workdir>/contamination.illumina.*`` and / or ``contamination.pacbio.*`` and,
    with two BAMs, ``contamination.identity.txt``."""
    if not getattr(args, "contamination", False):
        return []
    from . import contamination as cn
    route = Route.from_args(args, need_ref=False)
    names = ("pacbio",) if route.pacbio else ("illumina", "pacbio")
    chromosomes = route.chromosomes or list(genome)
    sites = cn.read_sites(args.contamination_sites, genome, chromosomes)
    written: List[str] = []
    found = []
    for bam, name in zip(route.bams, names):
        stats: dict = {}
        got = cn.measure(bam, genome, chromosomes, sites, route.q_threshold, route.mapq_threshold, route.device, stats)
        found.append(got)
        written += got.write_all(os.path.join(args.workdir, "contamination." + name))
        total, est = got.total(), got.estimate()
        logging.getLogger("hello_amd.call").info(
            "--contamination %s: %d sites (%d records skipped), %d reads counting, %d observations, error rate %.4f, contamination "
            "%.3f [%.3f, %.3f] in %.2f s (BAM decode %.2f s, kernels %.1f ms)", name, total["n_sites"], sum(got.skipped.values()),
            total["counting"], total["observations"], est["error_rate"], est["k"] / 1000, est["k_lo"] / 1000, est["k_hi"] / 1000,
            stats.get("total_s", 0.0), stats.get("decode_s", 0.0), stats.get("sites_ms", 0.0) + stats.get("reads_ms", 0.0))
    if len(found) == 2:
        written.append(cn.write_identity(os.path.join(args.workdir, "contamination.identity.txt"), *found))
        logging.getLogger("hello_amd.call").info("--contamination identity: LOD %.3f over %d sites: %s", *cn.identity_of(*found))
    return written


SV_OPTIONS = ("sv_min_size", "sv_min_support", "sv_flank", "sv_cluster_gap", "sv_len_ratio")


def _sv_values(args) -> Tuple[int, int, int, int, float]:
    """(min_size, min_support, flank, cluster_gap, len_ratio): the --sv_* options given, else the defaults of ``hello_amd.sv``."""
    from . import sv
    defaults = (sv.MIN_SIZE, sv.MIN_SUPPORT, sv.FLANK, sv.CLUSTER_GAP, sv.LEN_RATIO)
    return tuple(d if getattr(args, flag, None) is None else getattr(args, flag) for flag, d in zip(SV_OPTIONS, defaults))


SV_PAIRS_OPTIONS = ("sv_pairs_library", "sv_pairs_k", "sv_clip_min")


def _sv_pairs_values(args) -> Tuple[int, int]:
    """(k, clip_min): --sv_pairs_k and --sv_clip_min where given, else the defaults of ``hello_amd.sv``."""
    from . import sv
    k, clip_min = getattr(args, "sv_pairs_k", None), getattr(args, "sv_clip_min", None)
    return (sv.PAIRS_K if k is None else k, sv.CLIP_MIN if clip_min is None else clip_min)


def check_sv(args) -> None:
    """The refusals of --sv and the --sv_* options, each naming the fix."""
    if not getattr(args, "sv", False):
        if getattr(args, "sv_split", False):
            raise SystemExit("--sv_split adds the split alignments to the pass over large deletions and insertions and there is none in "
                             "this run: add --sv, or drop --sv_split")
        if getattr(args, "sv_pairs", False):
            raise SystemExit("--sv_pairs adds the discordant read pairs to the pass over large deletions and insertions and there is none "
                             "in this run: add --sv, or drop --sv_pairs")
        for flag in SV_OPTIONS + SV_PAIRS_OPTIONS:
            if getattr(args, flag, None) is not None:
                raise SystemExit(f"--{flag} is an option of the pass over large deletions and insertions and there is none in this "
                                 f"run: add --sv, or drop --{flag}")
        return
    if not getattr(args, "sv_pairs", False):
        for flag in SV_PAIRS_OPTIONS:
            if getattr(args, flag, None) is not None:
                raise SystemExit(f"--{flag} is an option of the read pairs and this run looks at none: add --sv_pairs, or drop --{flag}")
    if args.shards:
        raise SystemExit("--sv reads the CIGARs of the reads of the BAM(s), and shard files hold reads that were fetched and filtered "
                         "before: drop --shards and start from the BAM with --from_bam or --from_bams, or drop --sv")
    if not _bam_route(args):
        raise SystemExit("--sv reads the CIGARs of the reads of the BAM(s), and this run has no BAM on its path: add --from_bam (one "
                         "BAM) or --from_bams (--ibam and --pbam), or drop --sv (python -m hello_amd.sv searches BAMs on their own)")
    if _several_processes(args):
        raise SystemExit("--sv runs its pass over the BAM(s) in one process on one GPU: run it with --gpus 1 as a plain command, or "
                         "drop --sv and run python -m hello_amd.sv on the BAM(s)")
    from . import sv
    sv.check_options(*_sv_values(args))
    if getattr(args, "sv_pairs", False):
        sv.library_option(args.sv_pairs_library, "sv_pairs_library")
        sv.check_pairs_options(*_sv_pairs_values(args), "sv_")


def sv_pass(args, genome: Dict[str, str], result_path: str) -> List[str]:
    """--sv: the large deletions and insertions of every BAM of the route at the route's --mapq_threshold and chromosomes -> the
    files written, ``<workdir>/sv.illumina.*`` and / or ``sv.pacbio.*``.  The reads' haplotypes: --haplotag_vcf, else the phased VCF
    --phase wrote beside ``result_path``, else the BAMs' HP tags."""
    if not getattr(args, "sv", False):
        return []
    from . import haplotag, sv
    route = Route.from_args(args, need_ref=False)
    names = ("pacbio",) if route.pacbio else ("illumina", "pacbio")
    min_size, min_support, flank, cluster_gap, len_ratio = _sv_values(args)
    phased = getattr(args, "haplotag_vcf", None) or (result_path[:-len(".vcf")] + ".phased.vcf" if getattr(args, "phase", False) else None)
    tagger = haplotag.Haplotagger(phased, route.chromosomes, route.q_threshold, route.mapq_threshold, route.device) if phased else None
    written: List[str] = []
    pairs = bool(getattr(args, "sv_pairs", False))
    pairs_k, clip_min = _sv_pairs_values(args)
    try:
        for bam, name in zip(route.bams, names):
            stats: dict = {}
            try:
                found = sv.measure(bam, genome, route.chromosomes or list(genome), tagger, min_size, flank, route.mapq_threshold, cluster_gap,
                                   sv.percent_of(len_ratio), min_support, device=route.device, stats=stats,
                                   split=bool(getattr(args, "sv_split", False)), pairs=pairs,
                                   library=sv.library_option(getattr(args, "sv_pairs_library", None), "sv_pairs_library") if pairs else None,
                                   k=pairs_k, clip_min=clip_min)
            except sv.LibraryError as refused:
                raise SystemExit("--sv_pairs %s: %s" % (name, refused)) from None
            written += found.write_all(os.path.join(args.workdir, "sv." + name))
            total = found.total()
            logging.getLogger("hello_amd.call").info(
                "--sv %s: %d reads counting, %d walked, %d signatures, %d events in %.2f s (BAM decode %.2f s, kernels %.1f ms; "
                "haplotypes from %s)", name, total["counting"], total["walked"], total["signatures"], total["candidates"],
                stats.get("total_s", 0.0), stats.get("decode_s", 0.0),
                sum(stats.get(k, 0.0) for k in sv.TIME_NAMES), phased or "the HP tags")
            if found.split:
                logging.getLogger("hello_amd.call").info(
                    "--sv_split %s: %d reads with an SA tag (%d malformed, %d with more than 7 entries), %d junctions, %d rows", name,
                    total["split_reads"], total["bad_sa"], total["too_many"], total["junctions"], total["split_signatures"])
            if found.pairs:
                logging.getLogger("hello_amd.call").info(
                    "--sv_pairs %s: library median %d, normal %d to %d (%s); %d pair-counted reads, %d rows (%d joined a cluster), %d "
                    "events from pairs alone, %d reads with a clipped end, %d reads with unusable mate fields", name, *found.library,
                    found.library_source, total["pair_reads"], total["pair_signatures"], total["pairs_assigned"],
                    total["pair_candidates"], total["clipped_reads"], total["bad_mate"])
    finally:
        if tagger is not None:
            tagger.close()
    return written


def run_resident(args) -> str:
    """--from_bam / --from_bams with --resident: hotspots and ``shard<N>.txt`` as ``shards_from_bam(s)`` write them, then ONE loop
    in this process: shard file -> candidate sites whose reads stay on the GPU (``candidates.resident_activity``) -> ``ShardScorer``
    (coalesced up to --sites_per_launch) -> record stage.  No read is written to disk and no ``<workdir>/shards`` exists; the
    candidate stage runs at the thresholds of the route without --resident, so both give the same bytes."""
    from . import candidates as cd, shard_pipeline as sp
    logger = logging.getLogger("hello_amd.call")
    check_resident(args)
    check_gvcf(args)
    check_phase(args)
    check_haplotag(args)
    check_qc(args)
    check_methylation(args)
    check_contamination(args)
    check_sv(args)
    route = Route.from_args(args)
    genome = read_fasta(route.ref, route.chromosomes)
    tagger = haplotagger_of(args, route)
    find, kw = route.finder(tagger)
    files = list(_shard_files(route.hotspot_args(args.workdir, genome)))
    features_dir = os.path.join(args.workdir, features_dir_name(args.ibam, args.pbam))
    os.makedirs(features_dir, exist_ok=True)
    wanted = set(route.chromosomes) if route.chromosomes else None
    threads = max(2, min(args.num_threads, len(os.sched_getaffinity(0))))

    from .loader import load
    network = load(args.network, device=args.device, arithmetic=getattr(args, "arithmetic", "fp32"))
    network.eval()
    network.providePredictions = True                  # caller_calling.py:865-868
    total: dict = {}

    def candidates_of(name):
        found = list(cd.resident_activity(list(route.bams), route.ref, name, genome=genome, find=find, total=total, **kw))
        if len(found) != 1:                             # _shard_files writes one chromosome per file
            raise ValueError(f"{name}: positions on {len(found)} chromosomes; a shard file holds one")
        logger.info("%s: %d sites", name, found[0].n_sites)
        return found[0]
    t0 = time.perf_counter()
    stats = sp.run(network, [name for _, name in files], lambda n: os.path.join(features_dir, "features%d" % n), args.include_hp,
                   _genome_bytes(genome), wanted, record_threads=max(1, threads - 1),
                   sites_per_launch=getattr(args, "sites_per_launch", 8192), tags=[n for n, _ in files], loader=candidates_of,
                   in_thread=True, annotate=getattr(args, "annotate", False), evidence=getattr(args, "annotate_evidence", False))
    evidence = _header_evidence(args, network)
    network.close()
    _close_haplotagger(tagger)
    logger.info("%d shard files, %d sites, %d reads in %d launches, %.2f s (candidate stage %.2f s of it, %.1f ms in its kernels; "
                "staging %.2f s, record stage %.2f s on its threads; resident set after the loop %.0f MB)", len(files), stats.sites,
                stats.reads, stats.launches, stats.seconds, stats.wait_read,
                sum(total.get(k, 0.0) for k in ("pass1_kernel_ms", "pass2_kernel_ms", "allele_kernel_ms", "clip_kernel_ms")),
                stats.stage_seconds, stats.record_seconds, _resident_mb())
    for out in stats.outputs:                           # call.py:225-229
        if SENTINEL not in open(out.prefix + ".log").read():
            raise ValueError("Did not run: log file %s doesn't have termination string" % (out.prefix + ".log"))
    result_path = os.path.join(args.workdir, "results.output.vcf")
    lengths = {c: len(g) for c, g in genome.items()}
    n = sp.merge_final_vcf(stats.outputs, lambda names: header(names, lengths, getattr(args, "annotate", False), evidence),
                           result_path)
    logger.info("Completed runs in %.2f s. %d records in %s", time.perf_counter() - t0, n, result_path)
    gvcf_pass(args, result_path, genome)
    phase_pass(args, result_path)
    qc_pass(args, genome)
    methylation_pass(args, genome, result_path)
    contamination_pass(args, genome)
    sv_pass(args, genome, result_path)
    return result_path


def main(args) -> str:
    logger = logging.getLogger("hello_amd.call")
    check_gvcf(args)
    check_phase(args)
    check_haplotag(args)
    check_mark_duplicates(args)
    check_qc(args)
    check_methylation(args)
    check_contamination(args)
    check_sv(args)
    if getattr(args, "mark_duplicates", False):
        return with_duplicates_marked(args)
    if getattr(args, "haplotag", False):
        return haplotag_passes(args)
    if getattr(args, "resident", False):
        return run_resident(args)
    if _bam_route(args) and not args.shards:
        flag, build = ("--from_bams", shards_from_bams) if getattr(args, "from_bams", False) else ("--from_bam", shards_from_bam)
        if getattr(args, "from_bam", False) and getattr(args, "from_bams", False):
            raise SystemExit("--from_bam (one BAM) and --from_bams (an Illumina and a PacBio BAM) exclude each other")
        if _under_launcher():
            raise SystemExit(f"{flag} under an external launcher would build the same shards in every rank: start it as a plain "
                             "command with --gpus N, or build the shards first and pass --shards")
        if getattr(args, "gpus", 1) > 1:
            # the ranks must start before this process touches the GPU (_launch_ranks): the BAM stages run in a child of their own
            import multiprocessing
            child = multiprocessing.get_context("spawn").Process(target=build, args=(args,))
            child.start()
            child.join()
            if child.exitcode != 0:
                raise SystemExit(f"the BAM stages of {flag} failed (exit status {child.exitcode})")
            args.shards = os.path.join(args.workdir, "shards")
        else:
            args.shards = build(args)
    if not args.shards:
        raise SystemExit("--shards is required: BAM / FASTA ingestion, hotspot detection and allele assembly are upstream of "
                         "this engine (SURVEY.md section 2, rows 9-13); extract candidate-site shards with the reference's "
                         "searcher and hello_amd.shards.write_shard")
    result_path = os.path.join(args.workdir, "results.output.vcf")
    under_launcher = _under_launcher()
    if getattr(args, "gpus", 1) > 1 and not under_launcher:
        rc = _launch_ranks(args)
        if rc != 0:
            raise SystemExit(rc)
        return result_path
    rank, world = (int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])) if under_launcher else (0, 1)
    local_rank = int(os.environ.get("LOCAL_RANK", rank))

    shard_paths = sorted((glob.glob(os.path.join(args.shards, "*.hshard")) + glob.glob(os.path.join(args.shards, "*.npz")))
                         if os.path.isdir(args.shards) else glob.glob(args.shards), key=natural_key)
    if not shard_paths:
        raise SystemExit(f"no shard matches {args.shards!r}")
    numbers = [shard_number(p, i) for i, p in enumerate(shard_paths)]
    if len(set(numbers)) != len(numbers):                # names that do not end in distinct numbers: number them in order
        numbers = list(range(len(shard_paths)))
    features_dir = os.path.join(args.workdir, features_dir_name(args.ibam, args.pbam))
    os.makedirs(features_dir, exist_ok=True)
    names = chromosome_list(args.chromosomes)
    wanted = set(names) if names else None
    genomes = read_fasta(args.ref, wanted) if args.ref else {}

    import torch
    from . import shard as sharding, shard_pipeline as sp
    lo, hi = 0, len(shard_paths)
    device = args.device
    threads = max(2, min(args.num_threads, len(os.sched_getaffinity(0))))
    if world > 1:
        import torch.distributed as dist
        device = local_rank % max(torch.cuda.device_count(), 1)
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
        threads = max(2, min(args.num_threads, len(sharding.pin_rank(local_rank, local_world, device))))
        # control plane only (shard totals, the end-of-run barrier): no tensor leaves a rank, so gloo serves every backend
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = shard_read_totals(shard_paths[rank::world], threads)
        gathered: List = [None] * world
        dist.all_gather_object(gathered, mine)
        totals = np.zeros(len(shard_paths), np.int64)
        for r, part in enumerate(gathered):
            totals[r::world] = part
        lo, hi = sharding.partition_sites(totals, world)[rank]
        logger.info("rank %d of %d: shards [%d, %d) of %d, %d reads of %d, GPU %d, %d host threads", rank, world, lo, hi,
                    len(shard_paths), int(totals[lo:hi].sum()), int(totals.sum()), device, threads)

    from .loader import load
    network = load(args.network, device=device, arithmetic=getattr(args, "arithmetic", "fp32"))
    network.eval()
    network.providePredictions = True                  # caller_calling.py:865-868
    readers = max(1, min(threads // 2, 8))
    t0 = time.perf_counter()
    stats = sp.run(network, shard_paths[lo:hi], lambda n: os.path.join(features_dir, "features%d" % n), args.include_hp,
                   _genome_bytes(genomes), wanted, reader_threads=readers, record_threads=max(1, threads - readers),
                   sites_per_launch=getattr(args, "sites_per_launch", 8192), tags=numbers[lo:hi],
                   annotate=getattr(args, "annotate", False), evidence=getattr(args, "annotate_evidence", False))
    evidence = _header_evidence(args, network)
    network.close()
    logger.info("rank %d: %d shards, %d sites, %d reads in %d launches, %.2f s (%.0f sites/s; waiting for readers %.2f s, "
                "staging %.2f s, record stage %.2f s on its threads; resident set after the loop %.0f MB)", rank, hi - lo,
                stats.sites, stats.reads, stats.launches, stats.seconds, stats.sites / max(stats.seconds, 1e-9), stats.wait_read,
                stats.stage_seconds, stats.record_seconds, _resident_mb())
    for out in stats.outputs:                           # call.py:225-229
        if SENTINEL not in open(out.prefix + ".log").read():
            raise ValueError("Did not run: log file %s doesn't have termination string" % (out.prefix + ".log"))
    outputs = stats.outputs
    if world > 1:
        import torch.distributed as dist
        sp.save_index(os.path.join(features_dir, "mean_index.rank%d.npz" % rank), outputs)
        dist.barrier()                                  # THE synchronisation of the run: every rank's files are complete
        if rank == 0:
            outputs = [o for r in range(world) for o in sp.load_index(os.path.join(features_dir, "mean_index.rank%d.npz" % r))]
    if rank == 0:
        lengths = {c: len(g) for c, g in genomes.items()}
        n = sp.merge_final_vcf(outputs, lambda names: header(names, lengths, getattr(args, "annotate", False), evidence), result_path)
        logger.info("Completed runs in %.2f s. %d records in %s", time.perf_counter() - t0, n, result_path)
        gvcf_pass(args, result_path, genomes)
        phase_pass(args, result_path)
        qc_pass(args, genomes)
        methylation_pass(args, genomes, result_path)
        contamination_pass(args, genomes)
        sv_pass(args, genomes, result_path)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return result_path


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s:%(message)s")
    main(parser().parse_args())
    sys.exit(0)
