"""ctypes binding of the BAM reader in libhello_mi355x.so (include/hello_mi355x.h: ``hello_bam_*``).

It stands in for the ``pysam.AlignmentFile.fetch`` the reference's read containers run per chunk
(python/PileupContainerLite.py:526-570).  It needs no engine, no model and no GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ._abi import ARRAY_GETTER, bind, check as _check, handle_array, i32, i64, vp

_ARRAYS = (  # (field, hello_bam_* selector, dtype)
    ("bases", 0, np.uint8), ("quals", 1, np.uint8), ("read_offsets", 2, np.int64), ("cigars", 3, np.uint32),
    ("cigar_offsets", 4, np.int64), ("ref_starts", 5, np.int64), ("ref_ends", 6, np.int64), ("mapq", 7, np.uint8),
    ("flags", 8, np.uint16), ("name_hash", 9, np.uint64), ("strand", 10, np.uint8), ("hp", 11, np.uint8),
)

_MOD_ARRAYS = (  # after hello_bam_fetch_mods
    ("deltas", 12, np.int32), ("probs", 13, np.uint8), ("offsets", 14, np.int64), ("mode", 15, np.uint8), ("state", 16, np.uint8),
)

_SA_ARRAYS = (("bytes", 17, np.uint8), ("offsets", 18, np.int64))  # after hello_bam_fetch_sa

_MATE_ARRAYS = (("tid", 19, np.int32), ("pos", 20, np.int64), ("tlen", 21, np.int32))  # after hello_bam_fetch_pairs, with the SA arrays

_PROTOTYPES = (
    ("hello_bam_open", [C.c_char_p, i32, C.POINTER(vp)]),
    ("hello_bam_n_references", [vp]),
    ("hello_bam_reference", [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64)]),
    ("hello_bam_fetch", [vp, C.c_char_p, i64, i64, i32, C.POINTER(vp)]),
    ("hello_bam_fetch_mods", [vp, C.c_char_p, i64, i64, i32, C.POINTER(vp)]),
    ("hello_bam_fetch_sa", [vp, C.c_char_p, i64, i64, i32, C.POINTER(vp)]),
    ("hello_bam_fetch_pairs", [vp, C.c_char_p, i64, i64, i32, C.POINTER(vp)]),
    ("hello_bam_reads_info", [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]),
    ("hello_bam_reads_array", ARRAY_GETTER),
    ("hello_bam_reads_free", [vp], None),
    ("hello_bam_close", [vp], None),
)


MARKS: dict = {}   # os.path.abspath of a BAM -> its markdup.Marks; filled by markdup.applied alone, empty without --mark_duplicates


def _lib():
    return bind(_PROTOTYPES)


@dataclass
class Reads:
    """One region's records in file order, as flat arrays (the layout ``hello_engine_featurize`` takes)."""
    bases: np.ndarray          # uint8 ASCII, all reads concatenated
    quals: np.ndarray          # uint8
    read_offsets: np.ndarray   # int64 [R + 1]
    cigars: np.ndarray         # uint32, BAM packing len << 4 | op
    cigar_offsets: np.ndarray  # int64 [R + 1]
    ref_starts: np.ndarray     # int64
    ref_ends: np.ndarray       # int64 (bam_endpos)
    mapq: np.ndarray           # uint8
    flags: np.ndarray          # uint16
    name_hash: np.ndarray      # uint64, FNV-1a of the read name
    strand: np.ndarray         # uint8, 1 = reverse
    hp: np.ndarray             # uint8, the HP integer tag, 0 when absent
    used_index: bool = False
    n_blocks: int = 0

    @property
    def n_reads(self) -> int:
        return int(self.ref_starts.shape[0])

    def pointers(self, extra: np.ndarray) -> List[int]:
        """The eleven leading arguments of an entry point that takes a read set: the ten arrays, then ``extra`` (hp or source)."""
        return [a.ctypes.data for a in (self.bases, self.quals, self.read_offsets, self.cigars, self.cigar_offsets, self.ref_starts,
                                        self.ref_ends, self.mapq, self.flags, self.name_hash, extra)]

    def read(self, i: int) -> Tuple[str, List[Tuple[int, int]], np.ndarray]:
        """(bases, [(op, length)], qualities) of read i."""
        a, b = int(self.read_offsets[i]), int(self.read_offsets[i + 1])
        cig = self.cigars[self.cigar_offsets[i]:self.cigar_offsets[i + 1]]
        return self.bases[a:b].tobytes().decode(), [(int(c) & 15, int(c) >> 4) for c in cig], self.quals[a:b]

    @staticmethod
    def concat(parts: List["Reads"]) -> Tuple["Reads", np.ndarray]:
        """All parts' reads one after the other, and the part (source) of every read."""
        def offsets(name):
            out, base = [np.zeros(1, np.int64)], 0
            for p in parts:
                o = getattr(p, name)
                out.append(o[1:] + base)
                base += int(o[-1])
            return np.concatenate(out)
        cat = {f: np.concatenate([getattr(p, f) for p in parts]) for f, _, _ in _ARRAYS if not f.endswith("offsets")}
        cat["read_offsets"], cat["cigar_offsets"] = offsets("read_offsets"), offsets("cigar_offsets")
        source = np.concatenate([np.full(p.n_reads, i, np.uint8) for i, p in enumerate(parts)])
        return Reads(**cat), source


@dataclass
class Mods:
    """The 5mC calls of one region's records (MM / ML tags), read for read beside a ``Reads``."""
    deltas: np.ndarray         # int32: per listed base the bases of its kind skipped before it, all reads concatenated
    probs: np.ndarray          # uint8: its ML byte
    offsets: np.ndarray        # int64 [R + 1]
    mode: np.ndarray           # uint8: 0 implicit ('.' or absent), 1 unknown ('?')
    state: np.ndarray          # uint8: 0 no modifications, 1 usable, 2 bad


@dataclass
class Splits:
    """The SA tags of one region's records, read for read beside a ``Reads``."""
    bytes: np.ndarray          # uint8: the text of every record's SA:Z tag without its NUL, all records concatenated
    offsets: np.ndarray        # int64 [R + 1]; a record without SA, or with SA of another type, has an empty range


@dataclass
class Mates:
    """The mate fields of one region's records, read for read beside a ``Reads``, as the records hold them."""
    tid: np.ndarray            # int32: next_refID
    pos: np.ndarray            # int64: next_pos, 0-based, -1 when absent
    tlen: np.ndarray           # int32: carried, used by no rule


class BamFile:
    """An open BAM: ``references`` from its header, ``fetch(chromosome, start, stop)`` -> ``Reads``.  Not thread-safe."""

    def __init__(self, path: str, threads: int = 16):
        self.path = path
        self._lib = _lib()
        h = C.c_void_p()
        _check(self._lib.hello_bam_open(os.fsencode(path), int(threads), C.byref(h)))
        self._h = h
        self.references: List[Tuple[str, int]] = []
        for i in range(self._lib.hello_bam_n_references(h)):
            name, length = C.c_char_p(), C.c_int64()
            _check(self._lib.hello_bam_reference(h, i, C.byref(name), C.byref(length)))
            self.references.append((name.value.decode(), int(length.value)))

    def fetch(self, chromosome: str, start: int = 0, stop: Optional[int] = None, use_index: Optional[bool] = None) -> Reads:
        """Records overlapping [start, stop).  use_index: None = the .bai when there is one, True = require it, False = scan."""
        return self._fetch(self._lib.hello_bam_fetch, chromosome, start, stop, use_index)[0]

    def fetch_with_mods(self, chromosome: str, start: int = 0, stop: Optional[int] = None,
                        use_index: Optional[bool] = None) -> Tuple[Reads, Mods]:
        """``fetch``, and the C+m calls of every record's MM / ML tags (never an error: a record's state says what was found)."""
        return self._fetch(self._lib.hello_bam_fetch_mods, chromosome, start, stop, use_index, True)

    def fetch_with_sa(self, chromosome: str, start: int = 0, stop: Optional[int] = None,
                      use_index: Optional[bool] = None) -> Tuple[Reads, Splits]:
        """``fetch``, and the text of every record's SA tag (never an error: a record without one has an empty range)."""
        return self._fetch(self._lib.hello_bam_fetch_sa, chromosome, start, stop, use_index, _SA_ARRAYS)

    def fetch_pairs(self, chromosome: str, start: int = 0, stop: Optional[int] = None,
                    use_index: Optional[bool] = None) -> Tuple[Reads, Splits, "Mates"]:
        """``fetch_with_sa``, and every record's mate fields (never an error: the values are what the record holds)."""
        return self._fetch(self._lib.hello_bam_fetch_pairs, chromosome, start, stop, use_index, _MATE_ARRAYS)

    def _fetch(self, entry, chromosome, start, stop, use_index, with_mods=False):
        if stop is None:
            stop = dict(self.references).get(chromosome, 0)
        r = C.c_void_p()
        _check(entry(self._h, chromosome.encode(), int(start), int(stop), -1 if use_index is None else int(bool(use_index)), C.byref(r)))
        try:
            n, used, blocks = C.c_int64(), C.c_int32(), C.c_int64()
            _check(self._lib.hello_bam_reads_info(r, C.byref(n), C.byref(used), C.byref(blocks)))
            out = {field: handle_array(self._lib.hello_bam_reads_array, r, which, dtype) for field, which, dtype in _ARRAYS}
            reads = Reads(**out, used_index=bool(used.value), n_blocks=int(blocks.value))
            if MARKS:                                   # markdup.applied: the duplicates of this BAM gain flag 0x400
                marks = MARKS.get(os.path.abspath(self.path))
                if marks is not None:
                    marks.apply(chromosome, reads)
            if not with_mods:
                return reads, None
            if with_mods is _MATE_ARRAYS:
                get = lambda table: {f: handle_array(self._lib.hello_bam_reads_array, r, which, dtype) for f, which, dtype in table}  # noqa: E731
                return reads, Splits(**get(_SA_ARRAYS)), Mates(**get(_MATE_ARRAYS))
            if with_mods is _SA_ARRAYS:
                return reads, Splits(**{field: handle_array(self._lib.hello_bam_reads_array, r, which, dtype) for field, which, dtype in _SA_ARRAYS})
            return reads, Mods(**{field: handle_array(self._lib.hello_bam_reads_array, r, which, dtype) for field, which, dtype in _MOD_ARRAYS})
        finally:
            self._lib.hello_bam_reads_free(r)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.hello_bam_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
