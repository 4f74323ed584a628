"""What the stages that take a BAM span after span share in Python: ``Handle``, the base of the classes that bind a library handle
(close, context-manager use, ``stats`` and ``arrays`` from a table); ``measure_spans``, the pass over one BAM and its reference that
``qc.measure``, ``methylation.measure`` and ``contamination.measure`` are calls of; ``span_step`` and ``adder``, which the passes
with a loop of their own (markdup, phase, gvcf: DESIGN.md section 7o) share; and ``save_tables``, the deterministic npz."""
from __future__ import annotations

import ctypes as C
import io
import time
import zipfile
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

from ._abi import handle_array, handle_stats


def span_step(max_span: Optional[int]) -> int:
    """The positions of a span: ``max_span``, or what one launch takes."""
    from .hotspots import MAX_LAUNCH_BASES
    return int(max_span or MAX_LAUNCH_BASES)


def adder(stats: Optional[dict]) -> Callable[[str, float], None]:
    """``add(key, value)`` into ``stats``; nothing where there is none."""
    if stats is None:
        return lambda k, v: None
    return lambda k, v: stats.__setitem__(k, stats.get(k, 0.0) + v)


class Handle:
    """A ``hello_<NAME>`` handle of the library ``lib``: ``self._h`` is filled by the subclass (at once, or by its first add).
    ARRAYS: (name, selector, dtype, shape or None) per array; STAT_NAMES: the statistics; TIMES: those that are kernel times."""
    NAME = ""
    ARRAYS: Sequence[Tuple[str, int, object, Optional[tuple]]] = ()
    STAT_NAMES: Sequence[str] = ()
    TIMES: Sequence[str] = ()

    def __init__(self, lib):
        self._lib, self._h = lib, C.c_void_p()

    def _fn(self, what: str):
        return getattr(self._lib, "hello_%s_%s" % (self.NAME, what))

    def _array(self, which: int, dtype) -> np.ndarray:
        return handle_array(self._fn("array"), self._h, which, dtype)

    def _has(self, name: str) -> bool:
        """Whether array ``name`` exists yet (some do after a finishing call only)."""
        return True

    def arrays(self) -> Dict[str, np.ndarray]:
        return {name: self._array(which, dtype).reshape(shape) if shape else self._array(which, dtype)
                for name, which, dtype, shape in self.ARRAYS if self._has(name)}

    def stats(self) -> Dict[str, float]:
        return handle_stats(self._fn("stats"), self._h, self.STAT_NAMES)

    def results(self) -> Tuple[Dict[str, np.ndarray], Dict[str, float]]:
        """After the last add: (arrays, statistics)."""
        return self.arrays(), self.stats()

    def close(self) -> None:
        if self._h:
            self._fn("free")(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def measure_spans(bam: str, fasta, chromosomes: Optional[Sequence[str]], max_span: Optional[int], stats: Optional[dict],
                  restatement: bool, *, open_handle: Callable, restated: Callable, done: Callable, with_mods: bool = False,
                  retag: Optional[Callable] = None, with_sa: bool = False, with_pairs: bool = False) -> None:
    """One BAM, chromosome after chromosome (default: every sequence of ``fasta``, a path or {chromosome: sequence}), each in spans
    of ``span_step(max_span)`` positions.  Per chromosome ``c`` with its text ``ref`` (uint8):

    ``open_handle(c, ref)`` -> the ``Handle`` whose ``add(reads[, mods], lo, hi)`` takes every span and whose ``results()`` are
    read after the last; it is closed on every path.  It is not called under ``restatement``, and where it returns None the
    chromosome is restated too: the spans are collected and ``restated(c, ref, [(reads[, mods], lo, hi)])`` -> (tables, counts).  Either pair
    goes to ``done(c, ref, tables, counts)``.  ``with_mods``: the reads come with their modifications (``fetch_with_mods``);
    ``with_sa``: with their SA tags (``fetch_with_sa``); ``with_pairs``: with their SA tags and mate fields (``fetch_pairs``);
    ``retag(c, reads)`` replaces the reads of a span.  Added to ``stats``: the handle's TIMES, the seconds of decoding
    (``decode_s``), of the library's calls (``device_s``) and of the whole pass (``total_s``)."""
    from .bam import BamFile
    from .gvcf import _bytes_of
    if isinstance(fasta, str):
        from .call import read_fasta
        genome = read_fasta(fasta, chromosomes)
    else:
        genome = fasta
    step, add = span_step(max_span), adder(stats)
    t_all = time.perf_counter()
    with BamFile(bam) as source:
        known = dict(source.references)
        for c in (chromosomes or list(genome)):
            if c not in genome or c not in known:
                raise ValueError(f"no sequence named {c!r} in the " + ("BAM header" if c in genome else "reference"))
            ref = np.ascontiguousarray(_bytes_of(genome[c]))
            if ref.shape[0] != known[c]:
                raise ValueError(f"{c}: {ref.shape[0]} bases in the reference, {known[c]} in the BAM header")
            spans = []
            t0 = time.perf_counter()
            handle = None if restatement else open_handle(c, ref)
            add("device_s", time.perf_counter() - t0)
            try:
                for lo in range(0, ref.shape[0], step):
                    hi = min(lo + step, ref.shape[0])
                    t0 = time.perf_counter()
                    batch = (tuple(source.fetch_with_mods(c, lo, hi)) if with_mods else tuple(source.fetch_pairs(c, lo, hi)) if with_pairs
                             else tuple(source.fetch_with_sa(c, lo, hi)) if with_sa else (source.fetch(c, lo, hi),))
                    t1 = time.perf_counter()
                    if retag is not None:
                        batch = (retag(c, batch[0]),) + batch[1:]
                    if handle is None:
                        spans.append(batch + (lo, hi))
                    else:
                        handle.add(*batch, lo, hi)
                    add("decode_s", t1 - t0)
                    add("device_s", time.perf_counter() - t1)
                t0 = time.perf_counter()
                if handle is None:
                    tables, counts = restated(c, ref, spans)
                else:
                    tables, counts = handle.results()
                    for k in handle.TIMES:
                        add(k, counts[k])
                add("device_s", time.perf_counter() - t0)
            finally:
                if handle is not None:
                    handle.close()
            done(c, ref, tables, counts)
    add("total_s", time.perf_counter() - t_all)


def save_tables(path: str, tables: Dict[str, object]) -> str:
    """``np.savez``'s layout with a fixed time stamp: the same tables give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in tables.items():
            data = io.BytesIO()
            np.lib.format.write_array(data, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), data.getvalue())
    return path
