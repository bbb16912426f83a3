"""The compiled upstream IASP decoder (decoder id 5), where oracle/_ref exists.

oracle/ref_driver.cpp's ref_decode does not dispatch id 5, but ref_open(5, ...) opens a working IASP state (decod_open +
decod_init) and the library exports isum_prod_gf2_decod_qc_lm itself, so the decoder is called directly with our own
soft[] / decword[] buffers.  Test infrastructure only.
"""
import ctypes as C

import numpy as np

from ldpc_testlib import IASP_DEC, _as_double_p, c_double_p, c_short_p, ref_lib

_SYM = "_Z25isum_prod_gf2_decod_qc_lmP9DEC_STATEPdS1_ii"   # int isum_prod_gf2_decod_qc_lm(DEC_STATE*, double*, double*, int, int)


def iasp_ref_available():
    lib = ref_lib()
    return lib is not None and hasattr(lib, _SYM)


class IaspReference:
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
        self.h = self.lib.ref_open(IASP_DEC, self.rh, self.nh, M, H.ctypes.data_as(c_short_p))
        assert self.h

    def decode(self, llr, maxiter, decision=1):
        """llr [B, N] -> (decword [B, N], iters [B], soft[] as the decoder left it [B, N])."""
        llr = np.atleast_2d(np.ascontiguousarray(llr, dtype=np.float64))
        B, N = llr.shape
        assert N == self.N
        after = llr.copy()
        dec = np.empty((B, N), dtype=np.float64)
        its = np.empty(B, dtype=np.int32)
        for b in range(B):
            row = np.ascontiguousarray(after[b])
            out = np.empty(N, dtype=np.float64)
            its[b] = self.fn(self.h, _as_double_p(row), _as_double_p(out), maxiter, decision)
            after[b] = row
            dec[b] = out
        return dec, its, after

    def close(self):
        if self.h:
            self.lib.ref_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
