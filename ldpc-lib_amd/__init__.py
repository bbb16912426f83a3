"""ldpc-lib_amd: MI355X-native batched QC-LDPC belief-propagation decoding behind the call surface of
eovs/ldpc-lib's `decoders.h` / `bp_simulation.h`.

The product is the C-ABI shared library `libldpc_hip.so` (include/ldpc_hip.h) built from csrc/*.hip for gfx950,
plus the C++ source-compatible layer (include/ldpc/*.h, csrc/compat/*.cpp).  This Python package is only the
thin ctypes binding that tests/ and bench.py use (and a reference for other FFI users); PyTorch is used by the
callers for device memory, streams and torch.distributed -- never for the arithmetic.

There is deliberately no CPU fallback: importing works anywhere, but every compute entry point raises
`LdpcHipError` when the HIP library or a GPU is missing.
"""
from .binding import (DEC_ASP, DEC_BP, DEC_FHT, DEC_IASP, DEC_IMS, DEC_LCHE, DEC_LMS, DEC_MS, DEC_SP, DEC_TASP, LdpcHip, LdpcHipCodes, LdpcHipCodesGfq, LdpcHipError, LdpcHipGfq, LdpcHipMulti, build_library, codes_gfq_table, codes_table, gfq_left2right, gfq_upstream_message, girth_codes, girth_graph, check_voltages, failed_moduli, label_bank, label_codes, label_equations, label_last_stats, library_path, trace_matrix,  # noqa: F401
                      load_library)
from .host import GpuFrameSource, MtFrameSource, bp_simulation, bp_simulation_codes, mt19937_state, relift_base_matrix, replay_stop_rule, replay_stopping_rule  # noqa: F401

__all__ = ["LdpcHip", "LdpcHipCodes", "codes_table", "LdpcHipCodesGfq", "codes_gfq_table", "LdpcHipGfq", "gfq_left2right", "gfq_upstream_message", "LdpcHipError", "DEC_FHT", "DEC_BP", "DEC_SP", "DEC_ASP", "DEC_MS", "DEC_IMS", "DEC_IASP", "DEC_TASP", "DEC_LMS", "DEC_LCHE", "build_library", "library_path",
           "load_library", "girth_codes", "girth_graph", "trace_matrix", "label_equations", "label_codes", "label_last_stats", "check_voltages", "failed_moduli", "label_bank", "bp_simulation", "bp_simulation_codes", "relift_base_matrix", "replay_stop_rule"]
