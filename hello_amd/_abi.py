"""The ctypes plumbing every BAM-side stage module repeats: binding a table of prototypes, turning a status into an exception with
``hello_last_error``, and copying a handle's (pointer, count) arrays and statistics out.  ``engine.py`` and ``shared.py`` format
their own status messages and do not come through here."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np

from .engine import load_library

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
READS = [vp] * 11                  # the leading arguments of an entry point that takes a read set (bam.Reads.pointers)
ARRAY_GETTER = [vp, i32, C.POINTER(vp), C.POINTER(i64)]
STATS_GETTER = [vp, C.POINTER(C.c_double)]

_bound = set()


def bind(prototypes):
    """The library with every ``(name, argtypes[, restype])`` of the table bound, once per process (restype: int unless given)."""
    lib = load_library()
    for name, argtypes, *restype in prototypes:
        if name not in _bound:
            fn = getattr(lib, name)
            fn.argtypes = list(argtypes)
            if restype:
                fn.restype = restype[0]
            _bound.add(name)
    return lib


def check(rc: int, value_error_on_arg: bool = False) -> None:
    """Raise the library's last error for a non-zero status: RuntimeError, or ValueError for HELLO_ERR_ARG where asked."""
    if rc != 0:
        message = load_library().hello_last_error().decode(errors="replace")
        raise (ValueError if value_error_on_arg and rc == -1 else RuntimeError)(message)


def handle_array(getter, handle, which: int, dtype, *prefix) -> np.ndarray:
    """An owned copy of array ``which`` of ``handle``; ``prefix``: what the getter takes between the two (a technology)."""
    p, n = C.c_void_p(), C.c_int64()
    check(getter(handle, *prefix, which, C.byref(p), C.byref(n)))
    k = int(n.value)
    if k == 0:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (k * np.dtype(dtype).itemsize)).from_address(p.value), dtype).copy()


def handle_stats(getter, handle, names: Sequence[str]) -> Dict[str, float]:
    st = (C.c_double * len(names))()
    check(getter(handle, st))
    return dict(zip(names, list(st)))
