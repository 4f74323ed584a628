"""BAM records with mate fields, for the tests of the read pairs.  tests/bam_writer.py writes -1, -1, 0 into
``next_refID``, ``next_pos`` and ``tlen``; here its encoded record is taken as it is and those twelve bytes of the fixed core are
patched.  Blocks, index and file layout are ``bam_writer``'s own."""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Sequence, Tuple
from unittest import mock

from tests import bam_writer
from tests.bam_writer import Read

_CORE_AT = 4 + 20            # behind block_size: refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq take 20 bytes


@dataclass
class MatedRead(Read):
    next_ref_id: int = -1
    next_pos: int = -1
    tlen: int = 0


def encode_record(r: Read) -> bytes:
    """``bam_writer.encode_record`` with the record's own mate fields in place."""
    raw = bytearray(_plain_encode(r))
    if isinstance(r, MatedRead):
        raw[_CORE_AT:_CORE_AT + 12] = struct.pack("<iii", r.next_ref_id, r.next_pos, r.tlen)
    return bytes(raw)


_plain_encode = bam_writer.encode_record


def write_bam(path: str, references: Sequence[Tuple[str, int]], reads: Sequence[Read], index: bool = True, **kw) -> None:
    """``bam_writer.write_bam`` whose records carry their mate fields."""
    with mock.patch.object(bam_writer, "encode_record", encode_record):
        bam_writer.write_bam(path, references, reads, index, **kw)
