"""Test-only BGZF / BAM / .bai writer (SAM/BAM format specification v1, sections 4.1-4.2, 5.1-5.2).

Records are written as given (the caller sorts them).  ``block_bytes`` bounds the uncompressed bytes of a BGZF block, so
small values put records across block boundaries.  ``write_bam(..., index=True)`` also writes ``<path>.bai`` with bins and
the 16 kbp linear index (missing windows filled with the previous offset, as htslib does).
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
_CODE_OF = np.full(256, 255, np.uint8)
_CODE_OF[np.frombuffer(SEQ_CODES.encode(), np.uint8)] = np.arange(16, dtype=np.uint8)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@dataclass
class Read:
    name: str
    pos: int                              # 0-based leftmost reference position
    cigar: List[Tuple[int, int]]          # [(op, length)], op codes of CIGAR_OPS
    seq: str
    qual: Optional[Sequence[int]]         # None: QUAL '*' (0xFF)
    flag: int = 0
    mapq: int = 60
    ref_id: int = 0
    tags: bytes = b""                     # encoded auxiliary fields, written before a CG tag

    @property
    def ref_end(self) -> int:
        """bam_endpos: leftmost position + reference length, at least + 1."""
        rlen = sum(n for op, n in self.cigar if op in (0, 2, 3, 7, 8))
        if (self.flag & 4) or rlen == 0:
            rlen = 1
        return self.pos + rlen

    @property
    def is_reverse(self) -> bool:
        return bool(self.flag & 16)


def cigar_string(cigar) -> str:
    return "".join(f"{n}{CIGAR_OPS[op]}" for op, n in cigar)


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def encode_record(r: Read) -> bytes:
    name = r.name.encode() + b"\0"
    l_seq = len(r.seq)
    codes = _CODE_OF[np.frombuffer(r.seq.encode(), np.uint8)]
    assert (codes < 16).all(), r.seq
    if l_seq % 2:
        codes = np.append(codes, 0)
    seq = (codes[0::2] << 4) | codes[1::2]
    qual = bytes([0xFF] * l_seq) if r.qual is None else bytes(r.qual)
    assert len(qual) == l_seq
    ops = np.array([n << 4 | op for op, n in r.cigar], "<u4")
    tags = r.tags
    if len(r.cigar) > 65535:                  # section 4.2.2: placeholder CIGAR, the real one in CG:B,I
        tags += b"CGBI" + struct.pack("<I", len(r.cigar)) + ops.tobytes()
        ops = np.array([l_seq << 4 | 4, (r.ref_end - r.pos) << 4 | 3], "<u4")
    body = struct.pack("<iiBBHHHiiii", r.ref_id, r.pos, len(name), r.mapq, reg2bin(r.pos, r.ref_end), len(ops), r.flag,
                       l_seq, -1, -1, 0) + name + ops.tobytes() + seq.astype(np.uint8).tobytes() + qual + tags
    return struct.pack("<i", len(body)) + body


def bgzf_block(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(data) + c.flush()
    bsize = len(payload) + 25
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + payload
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_bam(path: str, references: Sequence[Tuple[str, int]], reads: Sequence[Read], index: bool = True,
              block_bytes: int = 65280, eof: bool = True) -> None:
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in references)
    header = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(references))
    for n, l in references:
        header += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    stream = bytearray(header)
    starts = []
    for r in reads:
        starts.append(len(stream))
        stream += encode_record(r)
    ends = starts[1:] + [len(stream)]
    blocks, coffs, c = [], [], 0
    for i in range(0, len(stream), block_bytes):
        b = bgzf_block(bytes(stream[i:i + block_bytes]))
        blocks.append(b)
        coffs.append(c)
        c += len(b)
    coffs.append(c)

    def voff(u: int) -> int:
        k = u // block_bytes
        return (coffs[k] << 16) | (u - k * block_bytes)

    with open(path, "wb") as fh:
        for b in blocks:
            fh.write(b)
        if eof:
            fh.write(EOF_BLOCK)
    if index:
        write_bai(path + ".bai", len(references), reads, [voff(u) for u in starts], [voff(u) for u in ends])


def write_bai(path: str, n_refs: int, reads: Sequence[Read], vbeg: Sequence[int], vend: Sequence[int]) -> None:
    bins = [dict() for _ in range(n_refs)]
    linear = [dict() for _ in range(n_refs)]
    for r, b, e in zip(reads, vbeg, vend):
        if r.ref_id < 0:
            continue
        chunks = bins[r.ref_id].setdefault(reg2bin(r.pos, r.ref_end), [])
        if chunks and chunks[-1][1] == b:
            chunks[-1][1] = e
        else:
            chunks.append([b, e])
        for w in range(r.pos >> 14, ((r.ref_end - 1) >> 14) + 1):
            linear[r.ref_id][w] = min(linear[r.ref_id].get(w, b), b)
    out = bytearray(b"BAI\1" + struct.pack("<i", n_refs))
    for t in range(n_refs):
        out += struct.pack("<i", len(bins[t]))
        for bin_, chunks in sorted(bins[t].items()):
            out += struct.pack("<Ii", bin_, len(chunks))
            for b, e in chunks:
                out += struct.pack("<QQ", b, e)
        n_intv = max(linear[t]) + 1 if linear[t] else 0
        out += struct.pack("<i", n_intv)
        prev = 0
        for w in range(n_intv):
            prev = linear[t].get(w, prev)
            out += struct.pack("<Q", prev)
    with open(path, "wb") as fh:
        fh.write(out)
