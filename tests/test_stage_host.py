"""The host layer under the BAM-side stages, on the CPU: the two read walks of hello_amd/csrc/cigar.h as a stand-alone program under
AddressSanitizer and UBSan (tests/abi/cigar_check.cpp), the refusals of a malformed read through the real entry points of the built
library (they validate before they look for a device, so no GPU is needed), and the ctypes helper hello_amd/_abi.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from hello_amd import _abi, candidates, gvcf, hotspots, phase
from hello_amd.bam import Reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SHAPE = -1, -2
M, I, S = 0, 1, 4


def test_read_walks_are_clean_under_sanitizers(tmp_path):
    """cigar.h needs no HIP: the host compiler alone builds it, without a ROCm include path."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler on this box"
    exe = str(tmp_path / "cigar_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            os.path.join(ROOT, "tests", "abi", "cigar_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "cigar_check: ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])


def one_read(cigar, n_bases, ref_start=5, ref_end=None, flag=0, mapq=60, base="A"):
    """A read set of one read with the given (op, length) CIGAR and `n_bases` bases, whatever the CIGAR says."""
    ref_len = sum(n for op, n in cigar if op in (0, 2, 3, 7, 8))
    return Reads(bases=np.frombuffer((base * n_bases).encode(), np.uint8).copy(), quals=np.full(n_bases, 30, np.uint8),
                 read_offsets=np.array([0, n_bases], np.int64), cigars=np.array([n << 4 | op for op, n in cigar], np.uint32),
                 cigar_offsets=np.array([0, len(cigar)], np.int64), ref_starts=np.array([ref_start], np.int64),
                 ref_ends=np.array([ref_start + max(ref_len, 1) if ref_end is None else ref_end], np.int64),
                 mapq=np.array([mapq], np.uint8), flags=np.array([flag], np.uint16), name_hash=np.array([1], np.uint64),
                 strand=np.zeros(1, np.uint8), hp=np.zeros(1, np.uint8))


REFERENCE = np.frombuffer(b"ACGT" * 50, np.uint8)


def call_hotspots(r, source=0):
    lib, h = hotspots._lib(), C.c_void_p()
    starts, stops = np.array([0], np.int64), np.array([200], np.int64)
    rc = lib.hello_hotspots_find(*r.pointers(np.array([source], np.uint8)), 1, REFERENCE.ctypes.data, 200, starts.ctypes.data,
                                 stops.ctypes.data, 1, 0, 10, 10, 0, C.byref(h))
    return rc, lib.hello_last_error().decode(), h


def call_candidates(r, source=0):
    lib, h = candidates._lib(), C.c_void_p()
    positions = np.array([20], np.int64)
    rc = lib.hello_candidates_find(*r.pointers(r.hp), 1, REFERENCE.ctypes.data, 200, positions.ctypes.data, 1, 0, 150, 10, 10, 0,
                                   C.byref(h))
    return rc, lib.hello_last_error().decode(), h


def call_refblocks(r, source=0):
    lib, h = gvcf._lib(), C.c_void_p()
    rc = lib.hello_refblocks_find(*r.pointers(np.array([source], np.uint8)), 1, REFERENCE.ctypes.data, 200, 0, 200, None, None, 0,
                                  10, 10, 5, 0, 0, C.byref(h))
    return rc, lib.hello_last_error().decode(), h


# (entry point, the read, status, message): the messages as the sources spelled them before the walks were shared
REFUSALS = [
    (call_hotspots, dict(cigar=[(M, 5)], n_bases=4), ERR_SHAPE, "read 0: CIGAR query length 5, 4 bases"),
    (call_candidates, dict(cigar=[(M, 5)], n_bases=4), ERR_SHAPE, "read 0: CIGAR query length 5, 4 bases"),
    (call_refblocks, dict(cigar=[(M, 5)], n_bases=4), ERR_ARG, "read 0: its CIGAR consumes 5 bases, it has 4"),
    (call_hotspots, dict(cigar=[(M, 3), (9, 2)], n_bases=5), ERR_ARG, "read 0: CIGAR operation 9"),
    (call_candidates, dict(cigar=[(M, 3), (9, 2)], n_bases=5), ERR_ARG, "read 0: CIGAR operation 9"),
    (call_hotspots, dict(cigar=[(M, 3), (I, 0), (M, 2)], n_bases=5), ERR_ARG, "read 0: zero-length CIGAR operation"),
    (call_candidates, dict(cigar=[(M, 3), (I, 0), (M, 2)], n_bases=5), ERR_ARG, "read 0: zero-length CIGAR operation"),
    (call_hotspots, dict(cigar=[(M, 5)], n_bases=5, ref_end=11), ERR_SHAPE, "read 0: ref_end does not match its CIGAR"),
    (call_candidates, dict(cigar=[(M, 5)], n_bases=5, ref_end=11), ERR_SHAPE, "read 0: ref_end does not match its CIGAR"),
    (call_hotspots, dict(cigar=[(M, 5)], n_bases=5, base="Z"), ERR_ARG, "read 0: base 'Z' is not a BAM base code"),
    (call_candidates, dict(cigar=[(M, 5)], n_bases=5, base="Z"), ERR_ARG, "read 0: base 'Z' is not a BAM base code"),
    (call_candidates, dict(cigar=[(M, 3), (S, 2), (M, 3)], n_bases=8), ERR_ARG, "read 0: a soft clip between aligned operations"),
    (call_hotspots, dict(cigar=[(M, 5)], n_bases=5, source=3), ERR_ARG, "source[0] = 3 with 1 read set(s)"),
    (call_refblocks, dict(cigar=[(M, 5)], n_bases=5, source=3), ERR_ARG, "source[0] = 3: 0 or 1"),
]


@pytest.mark.parametrize("entry,read,status,message", REFUSALS, ids=["%s-%s" % (r[0].__name__[5:], r[3][8:30].strip()) for r in REFUSALS])
def test_entry_points_refuse_a_malformed_read_before_they_look_for_a_device(entry, read, status, message):
    read = dict(read)
    source = read.pop("source", 0)
    rc, said, handle = entry(one_read(**read), source)
    assert (rc, said) == (status, message)
    assert not handle.value


def test_reads_a_stage_does_not_use_are_not_looked_at():
    """The same malformed read, unmapped: the hotspot and candidate stages skip it, the reference blocks skip a QC-fail read.  What
    the stages answer then needs a device or needs none; either way it is not the refusal of the read."""
    for entry, flag in ((call_hotspots, 0x4), (call_candidates, 0x4), (call_refblocks, 0x200)):
        rc, said, handle = entry(one_read([(M, 5)], 4, flag=flag))
        assert "read 0" not in said or rc == 0, (entry.__name__, rc, said)
        if rc == 0:
            free = {call_hotspots: "hello_hotspots_free", call_candidates: "hello_candidates_free", call_refblocks: "hello_refblocks_free"}
            getattr(hotspots._lib(), free[entry])(C.c_void_p(handle.value))


# ---- the binding helper -------------------------------------------------------------------------------------------------------
class FakeHandle:
    """A getter in the shape of hello_*_array over arrays held here, so that ownership can be seen without a device."""

    def __init__(self, arrays):
        self.arrays = arrays

    def getter(self, handle, *args):
        *prefix, which, p, n = args
        a = self.arrays[(tuple(prefix), which)]
        p._obj.value, n._obj.value = (a.ctypes.data if a.size else None), a.size
        return 0


def test_handle_array_copies_out_of_a_live_handle(tmp_path):
    """A real handle that needs no device: the reads of a BAM region.  The copy is the caller's; the handle's memory is not."""
    from hello_amd import bam
    from tests.bam_writer import Read, write_bam
    path = str(tmp_path / "two.bam")
    write_bam(path, [("chr1", 1000)], [Read("a", 10, [(M, 4)], "ACGT", [30] * 4), Read("b", 12, [(M, 3), (I, 1), (M, 2)], "ACGTAC", [20] * 6)])
    with bam.BamFile(path) as f:
        lib, r = bam._lib(), C.c_void_p()
        _abi.check(lib.hello_bam_fetch(f._h, b"chr1", 0, 1000, -1, C.byref(r)))
        try:
            cigars = _abi.handle_array(lib.hello_bam_reads_array, r, 3, np.uint32)
            assert cigars.dtype == np.uint32 and cigars.tolist() == [4 << 4, 3 << 4, 1 << 4 | 1, 2 << 4] and cigars.flags.owndata
            cigars[:] = 0
            assert _abi.handle_array(lib.hello_bam_reads_array, r, 3, np.uint32).tolist() == [4 << 4, 3 << 4, 1 << 4 | 1, 2 << 4]
            assert _abi.handle_array(lib.hello_bam_reads_array, r, 5, np.int64).tolist() == [10, 12]
            with pytest.raises(RuntimeError):                                     # the getter's status is checked
                _abi.handle_array(lib.hello_bam_reads_array, r, 99, np.uint8)
        finally:
            lib.hello_bam_reads_free(r)
        _abi.check(lib.hello_bam_fetch(f._h, b"chr1", 500, 600, -1, C.byref(r)))
        try:
            for which, dtype in ((0, np.uint8), (3, np.uint32), (5, np.int64), (8, np.uint16)):
                empty = _abi.handle_array(lib.hello_bam_reads_array, r, which, dtype)
                assert empty.dtype == dtype and empty.shape == (0,)
        finally:
            lib.hello_bam_reads_free(r)


def test_handle_array_with_a_getter_that_takes_a_technology():
    held = {((), 0): np.arange(5, dtype=np.int32), ((), 1): np.zeros(0, np.int64), ((1,), 0): np.arange(3, dtype=np.uint8)}
    fake = FakeHandle(held)
    first = _abi.handle_array(fake.getter, None, 0, np.int32)
    assert first.dtype == np.int32 and first.tolist() == [0, 1, 2, 3, 4] and first.flags.owndata and first.flags.writeable
    first[:] = -7
    assert held[((), 0)].tolist() == [0, 1, 2, 3, 4]
    assert _abi.handle_array(fake.getter, None, 0, np.int32).tolist() == [0, 1, 2, 3, 4]
    empty = _abi.handle_array(fake.getter, None, 1, np.int64)
    assert empty.dtype == np.int64 and empty.shape == (0,)
    assert _abi.handle_array(fake.getter, None, 0, np.uint8, 1).tolist() == [0, 1, 2]        # the technology goes before the selector


def test_check_and_the_chain_entry_point_through_the_helper():
    """hello_phase_chain is pure host: a refusal of it reaches Python as RuntimeError with the library's message, as ValueError only
    where the call site asks for that, and a status other than HELLO_ERR_ARG never does."""
    link = np.zeros((3, 2, 2), np.int32)
    link[1, 0] = [4, 0]
    link[2, 0] = [0, 4]
    sets, flip = phase.chain_native(link, window=2, min_margin=2)
    assert sets.tolist() == [0, 0, 0] and flip.tolist() == [0, 0, 1]
    assert phase.chain(link, window=2, min_margin=2)[0].tolist() == sets.tolist()
    with pytest.raises(RuntimeError, match="min_margin 0: at least 1") as refused:
        phase.chain_native(link, window=2, min_margin=0)
    assert not isinstance(refused.value, ValueError)
    lib = phase._lib()
    rc = lib.hello_phase_chain(link.ctypes.data, None, 3, 2, 2, None, None)
    assert rc == ERR_ARG
    with pytest.raises(ValueError, match="^NULL pointer$"):
        _abi.check(rc, value_error_on_arg=True)
    with pytest.raises(RuntimeError, match="^NULL pointer$") as plain:
        _abi.check(rc)
    assert not isinstance(plain.value, ValueError)
    with pytest.raises(RuntimeError) as shape:
        _abi.check(ERR_SHAPE, value_error_on_arg=True)
    assert not isinstance(shape.value, ValueError)
    _abi.check(0)
    _abi.check(0, value_error_on_arg=True)


def test_bind_sets_every_prototype_of_a_table_once():
    lib = _abi.bind(phase._PROTOTYPES)
    assert lib is _abi.bind(phase._PROTOTYPES) is phase._lib()
    assert lib.hello_phase_free.restype is None and lib.hello_phase_chain.restype is C.c_int
    assert len(lib.hello_phase_observe.argtypes) == 22 and lib.hello_phase_array.argtypes == _abi.ARRAY_GETTER
    r = one_read([(M, 5)], 5)
    assert r.pointers(r.hp) == [a.ctypes.data for a in (r.bases, r.quals, r.read_offsets, r.cigars, r.cigar_offsets, r.ref_starts,
                                                        r.ref_ends, r.mapq, r.flags, r.name_hash, r.hp)]
