"""The compiled upstream encode_NBQCLDPC and left2right, where oracle/_ref exists.

Like tests/gfq_ref.py: libldpc_ref.so's own C++ symbols through ctypes, on a DEC_STATE that GfqReference opened and initialised
(decod_open(FHT_DEC, ...), hb / hc / fht_ncols2convert, decod_init).  The byte offsets of DEC_STATE::codeword and ::syndr come from
the same kind of throwaway offsetof probe, compiled in a temporary directory against upstream's decoders.h; without the headers
there is no compiled encoder reference (the golden sets and the numpy model of tests/gfq_chain_model.py stand in).
Test infrastructure only.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from gfq_ref import GfqReference, _makefile_ref, gfq_ref_available
from ldpc_testlib import ref_lib

_ENCODE = "_Z15encode_NBQCLDPCP9DEC_STATEPi"   # int encode_NBQCLDPC(DEC_STATE *, int *)
_L2R = "_Z10left2rightPPsii"                   # void left2right(short **, int, int)
MEMBERS = ("codeword", "syndr")
_offsets = None


def _ref_dir():
    return os.environ.get("REF") or _makefile_ref()


def chain_ref_available():
    lib = ref_lib()
    return (gfq_ref_available() and all(hasattr(lib, s) for s in (_ENCODE, _L2R))
            and os.path.exists(os.path.join(_ref_dir(), "decoders.h")))


def member_offsets():
    global _offsets
    if _offsets is None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "probe.cpp")
            with open(src, "w") as f:
                f.write('#include <cstddef>\n#include <cstdio>\n#include "decoders.h"\nint main() {\n' +
                        "".join('  printf("%%zu\\n", offsetof(DEC_STATE, %s));\n' % m for m in MEMBERS) + "}\n")
            subprocess.check_call(["g++", "-DSKIP_MEX", "-w", "-I" + _ref_dir(), src, "-o", os.path.join(d, "probe")])
            _offsets = [int(v) for v in subprocess.check_output([os.path.join(d, "probe")]).decode().split()]
    return _offsets


def ref_left2right(matr):
    m = np.array(matr, dtype=np.int16, order="C")
    rows = (C.c_void_p * m.shape[0])(*[m[i].ctypes.data for i in range(m.shape[0])])
    fn = getattr(ref_lib(), _L2R)
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int]
    fn(rows, m.shape[0], m.shape[1])
    return m


class EncoderReference(GfqReference):
    def encode(self, msg):
        """msg [B, K] -> (codeword [B, N] int16 = st->codeword after the call, ok [B] = the return values).  A return of 0 before any
        work leaves the previous frame's codeword: callers that expect a refusal look at ok only."""
        fn = getattr(self.lib, _ENCODE)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p]
        o_cw, _ = member_offsets()
        cw_ptr = C.cast(C.c_void_p.from_address(self.h + o_cw).value, C.POINTER(C.c_int))
        cw_buf = np.ctypeslib.as_array(cw_ptr, shape=(self.N,))
        msg = np.ascontiguousarray(msg, dtype=np.int32)
        B = msg.shape[0]
        buf = np.zeros(self.N, dtype=np.int32)   # upstream's harness hands over n ints
        out = np.zeros((B, self.N), dtype=np.int16)
        ok = np.zeros(B, dtype=np.int32)
        for f in range(B):
            buf[:msg.shape[1]] = msg[f]
            ok[f] = fn(self.h, buf.ctypes.data)
            out[f] = cw_buf
        return out, ok
