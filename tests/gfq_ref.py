"""The compiled upstream GF(q) decoder (FHT_DEC, decoder id 6), where oracle/_ref exists.

oracle/ref_driver.cpp opens every state with q_bits = 1, so this module goes through libldpc_ref.so's own C++ symbols instead:
decod_open(FHT_DEC, q_bits, rh, nh, M), fill DEC_STATE::hb / hc / fht_ncols2convert, decod_init, and sum_prod_gfq_decod_lm per frame
with our own soft[] / qhard buffers; the a-posteriori vectors are read from DEC_STATE::fht_soft_out.  The byte offsets of those
members come from a throwaway offsetof probe compiled in a temporary directory against upstream's decoders.h; where the upstream
headers are absent (oracle/Makefile's REF), the offsets recorded in the golden sets (tools/make_gfq_goldens.py) are used.
Test infrastructure only.
"""
import ctypes as C
import glob
import os
import subprocess
import tempfile

import numpy as np

from ldpc_testlib import ORACLE_DIR, ref_lib

FHT_DEC = 6
_OPEN = "_Z10decod_openiiiii"                                  # DEC_STATE *decod_open(int, int, int, int, int)
_INIT = "_Z10decod_initPv"                                     # int decod_init(void *)
_CLOSE = "_Z11decod_closeP9DEC_STATE"                          # void decod_close(DEC_STATE *)
_DECODE = "_Z21sum_prod_gfq_decod_lmP9DEC_STATEPPdPsS2_id"     # int sum_prod_gfq_decod_lm(DEC_STATE *, double **, short *, double **, int, double)
MEMBERS = ("hb", "hc", "fht_ncols2convert", "fht_soft_out")
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfq")
_offsets = None


def gfq_ref_available():
    lib = ref_lib()
    return lib is not None and all(hasattr(lib, s) for s in (_OPEN, _INIT, _CLOSE, _DECODE))


def _makefile_ref():
    """Where oracle/Makefile looks for the upstream tree (its `REF ?=` default)."""
    with open(os.path.join(ORACLE_DIR, "Makefile")) as f:
        for line in f:
            if line.startswith("REF ?="):
                return line.split("=", 1)[1].strip()
    return ""


def member_offsets(ref_dir=None):
    """offsetof(DEC_STATE, m) for m in MEMBERS, of the compiled reference."""
    global _offsets
    if _offsets is not None:
        return _offsets
    ref_dir = ref_dir or os.environ.get("REF") or _makefile_ref()
    if os.path.exists(os.path.join(ref_dir, "decoders.h")):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "probe.cpp")
            with open(src, "w") as f:
                f.write('#include <cstddef>\n#include <cstdio>\n#include "decoders.h"\nint main() {\n' +
                        "".join('  printf("%%zu\\n", offsetof(DEC_STATE, %s));\n' % m for m in MEMBERS) + "}\n")
            subprocess.check_call(["g++", "-DSKIP_MEX", "-w", "-I" + ref_dir, src, "-o", os.path.join(d, "probe")])
            _offsets = [int(v) for v in subprocess.check_output([os.path.join(d, "probe")]).decode().split()]
    else:
        files = sorted(glob.glob(os.path.join(_GOLDEN, "*.npz")))
        assert files, "neither upstream's decoders.h nor a golden set to take the DEC_STATE offsets from"
        _offsets = [int(v) for v in np.load(files[0])["state_offsets"]]
    return _offsets


class GfqReference:
    def __init__(self, q_bits, hb, hc, M, ncols2convert=0):
        self.lib = ref_lib()
        assert self.lib is not None
        f_open, f_init = getattr(self.lib, _OPEN), getattr(self.lib, _INIT)
        self.f_close, self.fn = getattr(self.lib, _CLOSE), getattr(self.lib, _DECODE)
        f_open.restype = C.c_void_p
        f_open.argtypes = [C.c_int] * 5
        f_init.restype = C.c_int
        f_init.argtypes = [C.c_void_p]
        self.f_close.restype = None
        self.f_close.argtypes = [C.c_void_p]
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
        hb = np.ascontiguousarray(hb, dtype=np.int16)
        hc = np.ascontiguousarray(hc, dtype=np.int16)
        self.rh, self.nh = hb.shape
        self.q_bits, self.q, self.M = int(q_bits), 1 << int(q_bits), int(M)
        self.N = self.nh * self.M
        self.h = f_open(FHT_DEC, self.q_bits, self.rh, self.nh, self.M)
        assert self.h
        o_hb, o_hc, o_n2c, o_post = member_offsets()
        self._hc_rows = self._rows(o_hc)
        for rows, src in ((self._rows(o_hb), hb), (self._hc_rows, hc)):
            for j in range(self.rh):
                C.memmove(rows[j], src[j].ctypes.data, 2 * self.nh)
        C.c_int.from_address(self.h + o_n2c).value = int(ncols2convert)
        assert f_init(self.h), "decod_init failed"
        post_rows = C.cast(C.c_void_p.from_address(self.h + o_post).value, C.POINTER(C.c_void_p))
        self.post_bufs = [np.ctypeslib.as_array(C.cast(post_rows[s], C.POINTER(C.c_double)), shape=(self.N,)) for s in range(self.q)]

    def _rows(self, offset):
        pp = C.cast(C.c_void_p.from_address(self.h + offset).value, C.POINTER(C.c_void_p))
        return [pp[j] for j in range(self.rh)]

    def coefficients(self):
        """hc as decod_init left it."""
        out = np.empty((self.rh, self.nh), dtype=np.int16)
        for j in range(self.rh):
            C.memmove(out[j].ctypes.data, self._hc_rows[j], 2 * self.nh)
        return out

    def decode(self, soft, maxiter, p_thr=0.0):
        """soft [B, q, N] -> (iters [B], qhard [B, N] int16, post [B, q, N] = fht_soft_out, soft after the calls)."""
        soft = np.ascontiguousarray(soft, dtype=np.float64)
        if soft.ndim == 2:
            soft = soft[None]
        B = soft.shape[0]
        assert soft.shape[1:] == (self.q, self.N)
        after = soft.copy()
        iters = np.empty(B, dtype=np.int32)
        qhard = np.zeros((B, self.N), dtype=np.int16)
        post = np.empty_like(soft)
        dummy = np.zeros((self.q, self.N))
        for b in range(B):
            rows = (C.c_void_p * self.q)(*[after[b, s].ctypes.data for s in range(self.q)])
            drows = (C.c_void_p * self.q)(*[dummy[s].ctypes.data for s in range(self.q)])
            iters[b] = self.fn(self.h, rows, qhard[b].ctypes.data, drows, int(maxiter), float(p_thr))
            for s in range(self.q):
                post[b, s] = self.post_bufs[s]
        return iters, qhard, post, after

    def close(self):
        if self.h:
            self.f_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
