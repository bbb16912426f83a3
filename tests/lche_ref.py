"""The compiled upstream LCHE decoder (decoder id 9), where oracle/_ref exists.

oracle/ref_driver.cpp's ref_decode does not dispatch id 9, but ref_open(9, ...) opens a working LCHE state (decod_open +
decod_init) and the library exports lche_decod itself, so the decoder is called directly with our own soft[] / decword[]
buffers.  Upstream's only soft output is the state's lche_soft_out buffer (the final a-posteriori LLRs).  Its byte offset in
DEC_STATE is found by compiling a throwaway offsetof probe against upstream's decoders.h in a temporary directory; where the
upstream headers are absent (oracle/Makefile's REF), the offset recorded in the golden sets (tools/make_lche_goldens.py) is used.  Every frame checks
the buffer it reads: (soft < 0) == decword.  Test infrastructure only.
"""
import ctypes as C
import glob
import os
import subprocess
import tempfile

import numpy as np

from ldpc_testlib import LCHE_DEC, ORACLE_DIR, _as_double_p, c_double_p, c_short_p, ref_lib

_SYM = "_Z10lche_decodP9DEC_STATEPdS1_ii"   # int lche_decod(DEC_STATE*, double*, double*, int, int)
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lche")
_offset = None


def lche_ref_available():
    lib = ref_lib()
    return lib is not None and hasattr(lib, _SYM)


def _makefile_ref():
    """Where oracle/Makefile looks for the upstream tree (its `REF ?=` default)."""
    with open(os.path.join(ORACLE_DIR, "Makefile")) as f:
        for line in f:
            if line.startswith("REF ?="):
                return line.split("=", 1)[1].strip()
    return ""


def soft_out_offset(ref_dir=None):
    """offsetof(DEC_STATE, lche_soft_out) of the compiled reference."""
    global _offset
    if _offset is not None:
        return _offset
    ref_dir = ref_dir or os.environ.get("REF") or _makefile_ref()
    if os.path.exists(os.path.join(ref_dir, "decoders.h")):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "probe.cpp")
            with open(src, "w") as f:
                f.write('#include <cstddef>\n#include <cstdio>\n#include "decoders.h"\n'
                        'int main() { printf("%zu\\n", offsetof(DEC_STATE, lche_soft_out)); }\n')
            subprocess.check_call(["g++", "-DSKIP_MEX", "-w", "-I" + ref_dir, src, "-o", os.path.join(d, "probe")])
            _offset = int(subprocess.check_output([os.path.join(d, "probe")]).decode())
    else:
        files = sorted(glob.glob(os.path.join(_GOLDEN, "*.npz")))
        assert files, "neither upstream's decoders.h nor a golden set to take the lche_soft_out offset from"
        _offset = int(np.load(files[0])["soft_out_offset"])
    return _offset


class LcheReference:
    def __init__(self, H, M):
        self.lib = ref_lib()
        assert self.lib is not None
        self.fn = getattr(self.lib, _SYM)
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, c_double_p, c_double_p, C.c_int, C.c_int]
        H = np.ascontiguousarray(H, dtype=np.int16)
        self.rh, self.nh = H.shape
        self.M = M
        self.N = self.nh * M
        self.h = self.lib.ref_open(LCHE_DEC, self.rh, self.nh, M, H.ctypes.data_as(c_short_p))
        assert self.h
        ptr = C.c_void_p.from_address(self.h + soft_out_offset()).value
        self.soft_buf = np.ctypeslib.as_array(C.cast(ptr, c_double_p), shape=(self.N,))

    def decode(self, llr, maxiter, decision=0):
        """llr [B, N] -> (decword [B, N], iters [B], soft [B, N] = lche_soft_out, llr after the call [B, N])."""
        llr = np.atleast_2d(np.ascontiguousarray(llr, dtype=np.float64))
        B, N = llr.shape
        assert N == self.N
        after = llr.copy()
        dec = np.empty((B, N), dtype=np.float64)
        soft = np.empty((B, N), dtype=np.float64)
        its = np.empty(B, dtype=np.int32)
        for b in range(B):
            row = np.ascontiguousarray(after[b])
            out = np.empty(N, dtype=np.float64)
            its[b] = self.fn(self.h, _as_double_p(row), _as_double_p(out), maxiter, decision)
            after[b] = row
            dec[b] = out
            soft[b] = self.soft_buf
            assert np.array_equal((soft[b] < 0).astype(np.float64), dec[b]), "lche_soft_out does not match decword"
        return dec, its, soft, after

    def close(self):
        if self.h:
            self.lib.ref_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
