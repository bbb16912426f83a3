"""ctypes binding of the C-ABI in include/ldpc_hip.h (what cgo / JNI / any FFI would bind the same way).

Device buffers are torch CUDA tensors (torch = allocator + streams only); host entry points take numpy arrays laid
out exactly like the upstream per-frame arrays.
"""
import ctypes as C
import os
import subprocess

import numpy as np

# decoders.h:16-28 enum DEC_ID
DEC_BP, DEC_SP, DEC_ASP, DEC_MS, DEC_IMS, DEC_IASP, DEC_TASP, DEC_LMS, DEC_LCHE = 0, 1, 2, 3, 4, 5, 7, 8, 9
DEC_FHT = 6   # GF(q) codes: class LdpcHipGfq (ldpc_hip_open_gfq), not LdpcHip

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG_DIR)
_LIB_NAME = "libldpc_hip.so"
_lib = None
# hipcc flags of every translation unit of the library (build_library); tests that compile device code of their own against
# csrc/ import this list, so that they evaluate what the library evaluates.  -ffp-contract=off is part of the numerics contract.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I", os.path.join(_ROOT, "include")]


class LdpcHipError(RuntimeError):
    pass


def library_path():
    return os.path.join(_PKG_DIR, _LIB_NAME)


def build_library(force=False, verbose=False, jobs=None):
    """Compile csrc/ldpc_hip.hip (host side, table-driven / shape-unlimited / front-end / generator kernels) and csrc/aot/*.hip (the
    ahead-of-time code-specialised instances) for gfx950 -- one hipcc per translation unit, in parallel -- and link them into
    ldpc-lib_amd/libldpc_hip.so (in-tree, so it travels with the repo snapshot).
    -ffp-contract=off is part of the numerics contract: `y + s*alpha` must stay two roundings (decoders.cpp:4682)."""
    from concurrent.futures import ThreadPoolExecutor
    src_dir = os.path.join(_PKG_DIR, "csrc")
    aot_dir = os.path.join(src_dir, "aot")
    srcs = [os.path.join(src_dir, "ldpc_hip.hip")] + sorted(os.path.join(aot_dir, f) for f in os.listdir(aot_dir) if f.endswith(".hip"))
    headers = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith(".hpp")]
    headers += [os.path.join(_ROOT, "include", "ldpc_hip.h"), os.path.join(_ROOT, "include", "ldpc", "interleaver.h"),
                os.path.join(_ROOT, "include", "ldpc", "encoder.h")]
    aot_headers = [os.path.join(src_dir, f) for f in ("ldpc_aot.hpp", "ldpc_spec.hpp", "lche_table.hpp", "code_appendix_c_m64.hpp")]
    obj_dir = os.path.join(_PKG_DIR, "build")
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = HIPCC_FLAGS

    def newer(target, deps):
        return os.path.exists(target) and all(os.path.getmtime(d) <= os.path.getmtime(target) for d in deps)

    todo, objs = [], []
    for src in srcs:
        obj = os.path.join(obj_dir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        deps = [src] + (aot_headers if os.path.dirname(src) == aot_dir else headers)
        if force or not newer(obj, deps):
            todo.append([hipcc, *flags, "-c", src, "-o", obj])
    out = library_path()
    if not todo and newer(out, objs):
        return out

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, todo))
    run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", out])
    return out


def load_library():
    """Load libldpc_hip.so.  Raises LdpcHipError when it is missing -- there is no other compute path."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own ROCm runtime (libamdhip64).  Load torch FIRST so that this process has exactly one HIP
    # runtime and our library binds to the same one that owns torch's allocations and streams; loading ours first
    # pulls in /opt/rocm's copy and the second runtime then finds no device.
    try:
        import torch  # noqa: F401
        rtc = os.path.join(os.path.dirname(torch.__file__), "lib", "libhiprtc.so")
        if os.path.exists(rtc):  # JIT with the hiprtc that matches the HIP runtime torch brought into this process
            os.environ.setdefault("LDPC_HIP_HIPRTC_PATH", rtc)
        rccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(rccl):  # likewise one RCCL per process (ldpc_hip_open_multi dlopen()s it)
            os.environ.setdefault("LDPC_HIP_RCCL_PATH", rccl)
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise LdpcHipError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                           "There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, i64, f64, u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_double, C.c_uint64
    lib.ldpc_hip_abi_version.restype = i32
    lib.ldpc_hip_last_error.restype = C.c_char_p
    lib.ldpc_hip_device_count.restype = i32
    lib.ldpc_hip_open.argtypes = [i32, i32, i32, i32, vp, i32, C.POINTER(vp)]
    lib.ldpc_hip_close.argtypes = [vp]
    lib.ldpc_hip_close.restype = None
    for f in ("ldpc_hip_n", "ldpc_hip_r", "ldpc_hip_edges", "ldpc_hip_hard_words"):
        getattr(lib, f).argtypes = [vp]
    lib.ldpc_hip_kernel_name.argtypes = [vp]
    lib.ldpc_hip_last_launch.argtypes = [vp]
    lib.ldpc_hip_last_launch.restype = C.c_char_p
    lib.ldpc_hip_kernel_name.restype = C.c_char_p
    lib.ldpc_hip_decode_dev.argtypes = [vp, vp, i64, i32, f64, vp, vp, vp, vp]
    lib.ldpc_hip_decode_host.argtypes = [vp, vp, i64, i32, i32, f64, vp, vp, i32]
    lib.ldpc_hip_awgn_llr_dev.argtypes = [vp, f64, i32, i32, u64, i64, i64, vp, vp]
    lib.ldpc_hip_awgn_qam16_llr_dev.argtypes = [vp, f64, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_awgn_qam_llr_dev.argtypes = [vp, i32, f64, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_qam_demod_dev.argtypes = [i32, f64, f64, vp, i64, vp, i32, i32, vp]
    lib.ldpc_hip_count_errors_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.ldpc_hip_simulate.argtypes = [vp, f64, i32, i32, i32, f64, u64, i64, i64, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_set_bp_chain.argtypes = [vp, i32, i32]
    lib.ldpc_hip_set_ims_params.argtypes = [vp, f64, i32, i32]
    lib.ldpc_hip_encode_host.argtypes = [i32, i32, i32, vp, vp, vp]
    lib.ldpc_hip_interleaver_build.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.ldpc_hip_permute_dev.argtypes = [vp, vp, i64, i32, vp, i32, vp]
    lib.ldpc_hip_profile_enable.argtypes = [vp, i32]
    lib.ldpc_hip_profile_read.argtypes = [vp, C.POINTER(f64), C.POINTER(i64), i32]
    lib.ldpc_hip_set_interleaver.argtypes = [vp, i32, i32, i32]
    lib.ldpc_hip_set_codewords.argtypes = [vp, vp, i32]
    lib.ldpc_hip_channel_llr_dev.argtypes = [vp, f64, i32, i32, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_qam_modulate_dev.argtypes = [i32, vp, i64, vp, i32, vp]
    lib.ldpc_hip_count_errors_cw_dev.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp]
    lib.ldpc_hip_open_multi.argtypes = [i32, i32, i32, i32, vp, vp, i32, C.POINTER(vp)]
    lib.ldpc_hip_close_multi.argtypes = [vp]
    lib.ldpc_hip_close_multi.restype = None
    lib.ldpc_hip_multi_shards.argtypes = [vp]
    lib.ldpc_hip_multi_ctx.argtypes = [vp, i32]
    lib.ldpc_hip_multi_ctx.restype = vp
    lib.ldpc_hip_multi_reduction.argtypes = [vp]
    lib.ldpc_hip_multi_reduction.restype = C.c_char_p
    lib.ldpc_hip_multi_set_interleaver.argtypes = [vp, i32, i32, i32]
    lib.ldpc_hip_multi_set_codewords.argtypes = [vp, vp, i32]
    lib.ldpc_hip_simulate_multi.argtypes = [vp, f64, i32, i32, i32, f64, u64, i64, i64, i64, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_frames_multi.argtypes = [vp, f64, i32, i32, i32, f64, u64, i64, i64, i64, vp, vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_decode_host_multi.argtypes = [vp, vp, i64, i32, i32, f64, vp, vp, i32]
    lib.ldpc_hip_set_jit_mode.argtypes = [i32]
    lib.ldpc_hip_encode_dev.argtypes = [vp, vp, i64, vp, vp]
    lib.ldpc_hip_set_random_codewords.argtypes = [vp, u64, i32]
    lib.ldpc_hip_multi_set_random_codewords.argtypes = [vp, u64, i32]
    lib.ldpc_hip_mt_jump_host.argtypes = [vp, i32, vp]
    lib.ldpc_hip_mt_set_state.argtypes = [vp, vp, i32]
    lib.ldpc_hip_mt_get_state.argtypes = [vp, vp, C.POINTER(i32)]
    lib.ldpc_hip_mt_normal_dev.argtypes = [vp, i64, vp, vp]
    lib.ldpc_hip_mt_normal_host.argtypes = [vp, i64, vp]
    lib.ldpc_hip_mt_llr_dev.argtypes = [vp, f64, i32, i32, i64, vp, vp]
    lib.ldpc_hip_mt_frames.argtypes = [vp, f64, i32, i32, i32, f64, i64, vp, vp]
    lib.ldpc_hip_mt_frames_slice.argtypes = [vp, f64, i32, i32, i32, f64, i64, i64, i64, vp, vp]
    lib.ldpc_hip_set_jit_mode_thread.argtypes = [i32]
    lib.ldpc_hip_mt_set_frame_index.argtypes = [vp, i64]
    lib.ldpc_hip_mt_get_frame_index.argtypes = [vp]
    lib.ldpc_hip_mt_get_frame_index.restype = i64
    lib.ldpc_hip_multi_stream.argtypes = [vp, i32]
    lib.ldpc_hip_multi_stream.restype = vp
    lib.ldpc_hip_multi_comm_inits.restype = i64
    lib.ldpc_hip_multi_release_comms.restype = None
    lib.ldpc_hip_decode_count_multi.argtypes = [vp, vp, i64, i64, i32, f64, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_mt_set_state_multi.argtypes = [vp, vp, i32]
    lib.ldpc_hip_mt_get_state_multi.argtypes = [vp, vp, C.POINTER(i32)]
    lib.ldpc_hip_mt_set_frame_index_multi.argtypes = [vp, i64]
    lib.ldpc_hip_mt_advance_multi.argtypes = [vp, f64, i32, i32, i64]
    lib.ldpc_hip_mt_frames_multi.argtypes = [vp, f64, i32, i32, i32, f64, i64, vp, vp]
    lib.ldpc_hip_mt_shard_begin.argtypes = [vp, f64, i32, i32, i64, i32, i32, C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_mt_shard_emit.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(i32), vp, C.POINTER(i64)]
    lib.ldpc_hip_mt_shard_commit.argtypes = [vp, vp, i64, i32, f64, vp, vp]
    lib.ldpc_hip_mt_shard_abandon.argtypes = [vp]
    lib.ldpc_hip_mt_shard_abandon.restype = None
    lib.ldpc_hip_multi_mt_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    lib.ldpc_hip_multi_mt_stats.restype = None
    lib.ldpc_hip_open_gfq.argtypes = [i32, i32, i32, i32, vp, vp, i32, i32, C.POINTER(vp)]
    lib.ldpc_hip_gfq_q.argtypes = [vp]
    lib.ldpc_hip_gfq_coefficients.argtypes = [vp, vp]
    lib.ldpc_hip_decode_gfq_dev.argtypes = [vp, vp, i64, i32, f64, vp, vp, vp, vp]
    lib.ldpc_hip_decode_gfq_host.argtypes = [vp, vp, i64, i32, f64, vp, vp, vp]
    lib.ldpc_hip_gfq_left2right.argtypes = [vp, i32, i32]
    lib.ldpc_hip_gfq_k.argtypes = [vp]
    lib.ldpc_hip_gfq_sigma.argtypes = [vp, f64]
    lib.ldpc_hip_gfq_sigma.restype = f64
    lib.ldpc_hip_encode_gfq_dev.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.ldpc_hip_encode_gfq_host.argtypes = [vp, vp, i64, vp, vp]
    lib.ldpc_hip_gfq_channel_dev.argtypes = [vp, vp, vp, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_count_errors_gfq_dev.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    lib.ldpc_hip_simulate_gfq.argtypes = [vp, f64, i32, u64, i64, i64, i32, C.POINTER(C.c_ulonglong)]
    lib.ldpc_hip_gfq_upstream_message.argtypes = [i32, i32, vp]
    lib.ldpc_hip_gfq_set_codeword.argtypes = [vp, vp]
    lib.ldpc_hip_mt_set_state_gfq.argtypes = [vp, vp, i32]
    lib.ldpc_hip_mt_get_state_gfq.argtypes = [vp, vp, C.POINTER(i32)]
    lib.ldpc_hip_mt_advance_gfq.argtypes = [vp, i64]
    lib.ldpc_hip_mt_frames_gfq.argtypes = [vp, f64, i32, i32, i64, vp, vp]
    lib.ldpc_hip_frames_gfq_noise_host.argtypes = [vp, vp, f64, i32, i32, i64, vp, vp]
    for open_codes, open_id, codes_table_host, table_id in (_CODES_GENERIC, _CODES_WIDE, _CODES_GLOBAL, *_CODES_ROUTE.values()):
        getattr(lib, open_codes).argtypes = [i32] * open_id + [i32, i32, i32, vp, i32, i32, C.POINTER(vp)]
        getattr(lib, codes_table_host).argtypes = [i32] * table_id + [i32, i32, i32, vp, i32, vp, vp, i64, C.POINTER(i64)]
    lib.ldpc_hip_codes.argtypes = [vp]
    lib.ldpc_hip_decode_codes_dev.argtypes = [vp, vp, i32, i64, i32, f64, vp, vp, vp, vp]
    lib.ldpc_hip_count_errors_codes_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.ldpc_hip_simulate_codes.argtypes = [vp, f64, i32, i32, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_simulate_codes_stop.argtypes = [vp, f64, i32, i32, f64, u64, i64, i32, i64, f64, i64, i64, vp]
    lib.ldpc_hip_frames_codes_host.argtypes = [vp, vp, i64, i32, f64, vp, vp, vp]
    lib.ldpc_hip_mt_set_state_codes.argtypes = [vp, vp, i32]
    lib.ldpc_hip_mt_get_state_codes.argtypes = [vp, vp, C.POINTER(i32)]
    lib.ldpc_hip_mt_advance_codes.argtypes = [vp, f64, i32, i64]
    lib.ldpc_hip_mt_simulate_codes.argtypes = [vp, f64, i32, i32, f64, i64, vp, vp, vp]
    lib.ldpc_hip_mt_simulate_codes_stop.argtypes = [vp, f64, i32, i32, f64, i32, i64, f64, i64, i64, vp]
    lib.ldpc_hip_simulate_codes_grid.argtypes = [vp, vp, i32, i32, i32, f64, u64, i64, i64, vp, vp]
    lib.ldpc_hip_simulate_codes_grid_stop.argtypes = [vp, vp, i32, i32, i32, f64, u64, i64, i32, i64, vp, i64, i64, vp]
    lib.ldpc_hip_mt_simulate_codes_grid.argtypes = [vp, vp, i32, i32, i32, f64, i64, vp, vp, vp]
    lib.ldpc_hip_mt_simulate_codes_grid_stop.argtypes = [vp, vp, i32, i32, i32, f64, i32, i64, vp, i64, i64, vp]
    lib.ldpc_hip_open_codes_gfq.argtypes = [i32, i32, i32, i32, vp, vp, i32, i32, C.POINTER(vp)]
    lib.ldpc_hip_codes_gfq_table_host.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, C.POINTER(i64)]
    lib.ldpc_hip_decode_codes_gfq_dev.argtypes = [vp, vp, i32, i64, i32, vp, vp, vp, vp]
    lib.ldpc_hip_count_errors_codes_gfq_dev.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.ldpc_hip_simulate_codes_gfq.argtypes = [vp, f64, i32, u64, i64, i64, vp, vp]
    lib.ldpc_hip_simulate_codes_gfq_stop.argtypes = [vp, f64, i32, u64, i64, i32, i64, f64, i64, i64, vp]
    lib.ldpc_hip_codes_gfq_set_codewords.argtypes = [vp, vp]
    lib.ldpc_hip_mt_set_state_codes_gfq.argtypes = [vp, vp, i32]
    lib.ldpc_hip_mt_get_state_codes_gfq.argtypes = [vp, vp, C.POINTER(i32)]
    lib.ldpc_hip_mt_advance_codes_gfq.argtypes = [vp, i64]
    lib.ldpc_hip_mt_simulate_codes_gfq.argtypes = [vp, f64, i32, i32, i64, vp, vp, vp]
    lib.ldpc_hip_mt_simulate_codes_gfq_stop.argtypes = [vp, f64, i32, i32, i32, i64, f64, i64, i64, vp]
    lib.ldpc_hip_frames_codes_gfq_noise_host.argtypes = [vp, vp, f64, i32, i32, i64, vp, vp, vp]
    lib.ldpc_hip_girth_codes.argtypes = [i32, i32, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp]
    lib.ldpc_hip_girth_graph_host.argtypes = [i32, i32, i32, vp, C.POINTER(i32), vp, vp, C.POINTER(i64)]
    lib.ldpc_hip_label_equations_host.argtypes = [i32, i32, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), vp, vp, vp]
    lib.ldpc_hip_label_codes.argtypes = [i32, i32, vp, i32, i32, i64, i32, vp, i32, i32, vp, vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), vp,
                                         C.POINTER(i32)]
    lib.ldpc_hip_label_last_stats.argtypes = [vp]
    lib.ldpc_hip_check_voltages.argtypes = [i32, i32, vp, i32, i32, vp, vp, i64, i32, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    lib.ldpc_hip_label_bank.argtypes = [i32, i32, vp, i32, i32, i32, i64, i32, vp, i32, i32, vp, vp, vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), vp,
                                        C.POINTER(i32)]
    lib.ldpc_hip_label_last_stats.restype = None
    lib.ldpc_hip_trace_matrix_host.argtypes = [vp, vp, i32, C.POINTER(i32), vp, vp]
    if lib.ldpc_hip_abi_version() != 4:
        raise LdpcHipError("libldpc_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        raise LdpcHipError(f"{what}: {lib.ldpc_hip_last_error().decode()} (code {rc})")


def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(getattr(stream, "cuda_stream", stream))


class LdpcHip:
    """One opened code on one GPU == upstream's DEC_STATE (decod_open + hd fill + decod_init)."""

    def __init__(self, decoder_id, H, M, device=0):
        self.lib = load_library()
        H = np.ascontiguousarray(H, dtype=np.int16)
        self.rh, self.nh = H.shape
        self.M, self.decoder_id, self.device = int(M), int(decoder_id), int(device)
        h = C.c_void_p()
        rc = self.lib.ldpc_hip_open(self.decoder_id, self.rh, self.nh, self.M, H.ctypes.data, self.device, C.byref(h))
        _check(self.lib, rc, "ldpc_hip_open")
        self.h = h
        self.N = self.lib.ldpc_hip_n(h)
        self.R = self.lib.ldpc_hip_r(h)
        self.edges = self.lib.ldpc_hip_edges(h)
        self.hard_words = self.lib.ldpc_hip_hard_words(h)
        self._kernel_name = self.lib.ldpc_hip_kernel_name(h).decode()

    @property
    def kernel_name(self):
        """Kernel this context launches; with LDPC_HIP_JIT=async it changes once the background hiprtc instance is ready."""
        if getattr(self, "h", None):
            self._kernel_name = self.lib.ldpc_hip_kernel_name(self.h).decode()
        return self._kernel_name

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldpc_hip_close(self.h)
            self.h = None

    def last_launch(self):
        return self.lib.ldpc_hip_last_launch(self.h).decode()

    def set_ims_params(self, thr=1.4, qbits=6, dbits=8):
        """IMS_DEC: the quantiser arguments of imin_sum_decod_qc_lm (defaults MS_THR, MS_QBITS, MS_DBITS of decoders.h:46-48)."""
        _check(self.lib, self.lib.ldpc_hip_set_ims_params(self.h, float(thr), int(qbits), int(dbits)), "ldpc_hip_set_ims_params")

    def set_bp_chain(self, on=True, reset_carry=False):
        """BP_DEC: chain frames through upstream's uncleared syndrome array (include/ldpc_hip.h)."""
        _check(self.lib, self.lib.ldpc_hip_set_bp_chain(self.h, int(on), int(reset_carry)), "ldpc_hip_set_bp_chain")

    def set_interleaver(self, permutation_type, permutation_block=128, permutation_inter=1):
        """Bit interleaver between mapper / demapper and the code (permutation_type 0..4 of bp_simulation.h:21-23)."""
        _check(self.lib, self.lib.ldpc_hip_set_interleaver(self.h, int(permutation_type), int(permutation_block), int(permutation_inter)),
               "ldpc_hip_set_interleaver")

    def set_codewords(self, codewords):
        """Transmitted codewords uint8 [C, N] (frame f carries codeword f % C); None or empty = upstream's all-zero codeword."""
        if codewords is None or len(codewords) == 0:
            _check(self.lib, self.lib.ldpc_hip_set_codewords(self.h, None, 0), "ldpc_hip_set_codewords")
            return
        cw = np.ascontiguousarray(codewords, dtype=np.uint8).reshape(-1, self.N)
        _check(self.lib, self.lib.ldpc_hip_set_codewords(self.h, cw.ctypes.data, cw.shape[0]), "ldpc_hip_set_codewords")

    def set_random_codewords(self, seed, ncw):
        """ncw random codewords made on the device (Philox information bits + the device encoder); frame f carries codeword f % ncw."""
        _check(self.lib, self.lib.ldpc_hip_set_random_codewords(self.h, int(seed), int(ncw)), "ldpc_hip_set_random_codewords")

    def encode_dev(self, info_bits, stream=None):
        """uint8 CUDA tensor [B, (nh-rh)*M] of 0/1 -> codewords uint8 [B, N] (parity first), on the device."""
        import torch
        info = info_bits.contiguous()
        assert info.dtype == torch.uint8 and info.shape[1] == self.N - self.R
        out = torch.empty((info.shape[0], self.N), dtype=torch.uint8, device=info.device)
        rc = self.lib.ldpc_hip_encode_dev(self.h, C.c_void_p(info.data_ptr()), int(info.shape[0]), C.c_void_p(out.data_ptr()), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_encode_dev")
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- device-resident batch API -------------------------------------------------------------------
    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def decode(self, llr, maxiter, alpha=0.8, want_hard=True, want_soft=False, stream=None, out=None):
        """llr: torch float64 CUDA tensor [B,N] (not modified).  Returns (hard int32[B,W] | None, iters int32[B], soft | None).
        hard holds the packed uint32 words reinterpreted as int32 (torch has no uint32 arithmetic)."""
        import torch
        assert llr.is_cuda and llr.dtype == torch.float64 and llr.is_contiguous() and llr.shape[-1] == self.N
        B = llr.shape[0]
        if out is not None:
            hard, iters, soft = out
        else:
            hard = torch.empty((B, self.hard_words), dtype=torch.int32, device=llr.device) if want_hard else None
            iters = torch.empty((B,), dtype=torch.int32, device=llr.device)
            soft = torch.empty((B, self.N), dtype=torch.float64, device=llr.device) if want_soft else None
        rc = self.lib.ldpc_hip_decode_dev(self.h, llr.data_ptr(), B, int(maxiter), float(alpha),
                                          hard.data_ptr() if hard is not None else None, iters.data_ptr(),
                                          soft.data_ptr() if soft is not None else None, _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_decode_dev")
        return hard, iters, soft

    def awgn_llr(self, snr_db, seed, first_frame, B, modulation=0, punctured_blocks=0, out=None, stream=None, T=26.0):
        """Device-side channel: modulation 0 BPSK, 1 QAM4 (upstream formulas), 2 / 3 / 4 the 16- / 64- / 256-QAM chain (as intended upstream)."""
        import torch
        llr = out if out is not None else torch.empty((B, self.N), dtype=torch.float64, device=self._dev())
        rc = self.lib.ldpc_hip_channel_llr_dev(self.h, float(snr_db), int(modulation), int(punctured_blocks), float(T), int(seed),
                                               int(first_frame), int(B), llr.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_channel_llr_dev")
        return llr

    channel_llr = awgn_llr   # the whole chain: codeword -> interleaver -> mapper -> AWGN -> demapper -> interleaver -> puncturing

    def count_errors(self, hard, iters, counters=None, want_frame_info=False, stream=None, first_frame=0):
        """counters: int64 CUDA tensor[5] accumulated in place: nse, nde, nue, frames, sum|iters| (bp_simulation.cpp:805-810);
        hard decisions are compared with the codeword each frame carried (first_frame = global index of frame 0)."""
        import torch
        B = iters.shape[0]
        if counters is None:
            counters = torch.zeros(5, dtype=torch.int64, device=iters.device)
        info = torch.empty((B,), dtype=torch.int32, device=iters.device) if want_frame_info else None
        rc = self.lib.ldpc_hip_count_errors_cw_dev(self.h, hard.data_ptr(), iters.data_ptr(), int(first_frame), B,
                                                   info.data_ptr() if info is not None else None, counters.data_ptr(),
                                                   _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_count_errors_cw_dev")
        return counters, info

    def simulate(self, snr_db, maxiter, seed, first_frame, B, modulation=0, punctured_blocks=0, alpha=0.8):
        cnt = (C.c_ulonglong * 4)()
        sit = C.c_ulonglong()
        rc = self.lib.ldpc_hip_simulate(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(maxiter),
                                        float(alpha), int(seed), int(first_frame), int(B), cnt, C.byref(sit))
        _check(self.lib, rc, "ldpc_hip_simulate")
        return {"nse": cnt[0], "nde": cnt[1], "nue": cnt[2], "frames": cnt[3], "sum_abs_iters": sit.value}

    # ---- upstream's own mt19937 / normal_distribution noise stream on the device (exact replay) ----------
    def mt_set_state(self, state, pos):
        """state: 624 uint32 words + index of the next word, as libstdc++ streams a std::mt19937."""
        st = np.ascontiguousarray(state, dtype=np.uint32)
        assert st.shape == (624,)
        _check(self.lib, self.lib.ldpc_hip_mt_set_state(self.h, st.ctypes.data, int(pos)), "ldpc_hip_mt_set_state")

    def mt_get_state(self):
        st = np.empty(624, dtype=np.uint32)
        pos = C.c_int()
        _check(self.lib, self.lib.ldpc_hip_mt_get_state(self.h, st.ctypes.data, C.byref(pos)), "ldpc_hip_mt_get_state")
        return st, pos.value

    def mt_frame_index(self):
        """Frames drawn since mt_set_state (which codeword a frame carries: f % ncw); part of a generator snapshot."""
        return int(self.lib.ldpc_hip_mt_get_frame_index(self.h))

    def mt_set_frame_index(self, frames_taken):
        _check(self.lib, self.lib.ldpc_hip_mt_set_frame_index(self.h, int(frames_taken)), "ldpc_hip_mt_set_frame_index")

    def mt_normal(self, count, out=None, skip=False, stream=None):
        """The next `count` values of upstream's next_random_gaussian() (float64 CUDA tensor); skip=True draws and drops them."""
        import torch
        if not skip and out is None:
            out = torch.empty(int(count), dtype=torch.float64, device=self._dev())
        rc = self.lib.ldpc_hip_mt_normal_dev(self.h, int(count), None if skip else C.c_void_p(out.data_ptr()), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_mt_normal_dev")
        return out

    def mt_llr(self, snr_db, B, modulation=0, punctured_blocks=0, out=None, skip=False, stream=None):
        """Decoder input of the next B frames of upstream's frame loop ([B,N] float64 CUDA tensor); skip=True only advances."""
        import torch
        if not skip and out is None:
            out = torch.empty((int(B), self.N), dtype=torch.float64, device=self._dev())
        rc = self.lib.ldpc_hip_mt_llr_dev(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(B),
                                          None if skip else C.c_void_p(out.data_ptr()), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_mt_llr_dev")
        return out

    def mt_frames(self, snr_db, maxiter, B, modulation=0, punctured_blocks=0, alpha=0.8, lo=None, hi=None):
        """noise -> decode -> count for the next B frames: (frame_info, iters) int32 numpy arrays.  With lo / hi the generator still
        advances by all B frames but only frames [lo, hi) are decoded here (one rank's share when every rank runs the generator)."""
        lo = 0 if lo is None else int(lo)
        hi = int(B) if hi is None else int(hi)
        info = np.empty(max(hi - lo, 0), dtype=np.int32)
        its = np.empty(max(hi - lo, 0), dtype=np.int32)
        rc = self.lib.ldpc_hip_mt_frames_slice(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(maxiter), float(alpha), int(B),
                                               lo, hi, info.ctypes.data, its.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_frames_slice")
        return info, its

    # the generator's tape shared out over the ranks of a job, one process per GPU (ldpc_hip_mt_shard_*: the exchanges are the caller's)
    def mt_shard_begin(self, snr_db, frames, rank, n, modulation=0, punctured_blocks=0):
        own = C.c_ulonglong()
        _check(self.lib, self.lib.ldpc_hip_mt_shard_begin(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(frames), int(rank), int(n),
                                                          C.byref(own)), "ldpc_hip_mt_shard_begin")
        return own.value

    def mt_shard_emit(self, counts):
        cnt = np.ascontiguousarray(counts, dtype=np.uint64)
        found, covered, fdone = C.c_int(), C.c_int(), C.c_longlong()
        st = np.zeros(624, dtype=np.uint32)
        _check(self.lib, self.lib.ldpc_hip_mt_shard_emit(self.h, cnt.ctypes.data, C.byref(found), C.byref(covered), st.ctypes.data, C.byref(fdone)),
               "ldpc_hip_mt_shard_emit")
        return bool(found.value), bool(covered.value), st, fdone.value

    def mt_shard_commit(self, state, frames_done, maxiter, rows, alpha=0.8):
        st = np.ascontiguousarray(state, dtype=np.uint32)
        info = np.empty(max(int(rows), 0), dtype=np.int32)
        its = np.empty(max(int(rows), 0), dtype=np.int32)
        _check(self.lib, self.lib.ldpc_hip_mt_shard_commit(self.h, st.ctypes.data, int(frames_done), int(maxiter), float(alpha),
                                                           info.ctypes.data if rows > 0 else None, its.ctypes.data if rows > 0 else None), "ldpc_hip_mt_shard_commit")
        return info, its

    def mt_shard_abandon(self):
        self.lib.ldpc_hip_mt_shard_abandon(self.h)

    # ---- host-pointer API (upstream array layout, PCIe inclusive) --------------------------------------
    def decode_host(self, llr, maxiter, decision=0, alpha=0.8, clobber_sp_input=True):
        """llr: float64 [B,N] or [N].  Returns (decword, iters, llr_after) like the upstream decoder call: decword is
        0.0/1.0 (decision 0) or the a-posteriori values (decision 1); llr_after is what upstream leaves in its input
        array (unchanged for MS/LMS, the likelihood ratios for SP, decoders.cpp:1950,2124)."""
        llr = np.array(llr, dtype=np.float64, order="C", copy=True)
        single = llr.ndim == 1
        if single:
            llr = llr[None, :]
        B = llr.shape[0]
        assert llr.shape[1] == self.N
        dec = np.empty((B, self.N), dtype=np.float64)
        its = np.empty(B, dtype=np.int32)
        rc = self.lib.ldpc_hip_decode_host(self.h, llr.ctypes.data, B, int(maxiter), int(decision), float(alpha),
                                           dec.ctypes.data, its.ctypes.data, 1 if clobber_sp_input else 0)
        _check(self.lib, rc, "ldpc_hip_decode_host")
        if single:
            return dec[0], int(its[0]), llr[0]
        return dec, its, llr

    # ---- kernel timing (HIP events on the launch stream) ------------------------------------------------
    def profile(self, enable=True):
        _check(self.lib, self.lib.ldpc_hip_profile_enable(self.h, 1 if enable else 0), "ldpc_hip_profile_enable")

    def profile_read(self, reset=True):
        ms, n = C.c_double(), C.c_longlong()
        _check(self.lib, self.lib.ldpc_hip_profile_read(self.h, C.byref(ms), C.byref(n), 1 if reset else 0), "ldpc_hip_profile_read")
        return ms.value, n.value


def gfq_left2right(matr):
    """upstream's left2right (decoders.cpp:174-195) on a copy of the [rh, nh] matrix: columns rh .. nh-1, then rh-1, then 0 .. rh-2.
    bp_simulation.cpp:391-394 applies it to hb and hc before encoding."""
    m = np.array(matr, dtype=np.int16, order="C")
    assert m.ndim == 2
    lib = load_library()
    _check(lib, lib.ldpc_hip_gfq_left2right(m.ctypes.data, m.shape[0], m.shape[1]), "ldpc_hip_gfq_left2right")
    return m


def gfq_upstream_message(q_bits, K):
    """The message bp_simulation(q_mod > 2, ...) encodes, as include/ldpc_hip.h defines it: upstream's eight symbols {6, 11, 0, 4, 2, 1,
    2, 5} (the first K of them when K < 8), each reduced with & (q - 1), followed by zeros.  int16 [K]; no GPU needed."""
    msg = np.zeros(max(int(K), 0), dtype=np.int16)
    lib = load_library()
    _check(lib, lib.ldpc_hip_gfq_upstream_message(int(q_bits), int(K), msg.ctypes.data), "ldpc_hip_gfq_upstream_message")
    return msg


class LdpcHipGfq:
    """One opened QC-LDPC code over GF(q), q = 2^q_bits, on one GPU == upstream's DEC_STATE of decod_open(FHT_DEC, q_bits, ...) with hb,
    hc and fht_ncols2convert filled in and decod_init done.  hb: shifts (-1 empty), hc: coefficients 1 .. q-1 in natural representation."""

    def __init__(self, q_bits, hb, hc, M, ncols2convert=0, device=0):
        self.lib = load_library()
        hb = np.ascontiguousarray(hb, dtype=np.int16)
        hc = np.ascontiguousarray(hc, dtype=np.int16)
        assert hb.ndim == 2 and hb.shape == hc.shape
        self.rh, self.nh = hb.shape
        self.M, self.q_bits, self.device = int(M), int(q_bits), int(device)
        h = C.c_void_p()
        rc = self.lib.ldpc_hip_open_gfq(self.q_bits, self.rh, self.nh, self.M, hb.ctypes.data, hc.ctypes.data, int(ncols2convert), self.device, C.byref(h))
        _check(self.lib, rc, "ldpc_hip_open_gfq")
        self.h = h
        self.N = self.lib.ldpc_hip_n(h)
        self.R = self.lib.ldpc_hip_r(h)
        self.edges = self.lib.ldpc_hip_edges(h)
        self.q = self.lib.ldpc_hip_gfq_q(h)
        self.k = self.lib.ldpc_hip_gfq_k(h)
        self.kernel_name = self.lib.ldpc_hip_kernel_name(h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldpc_hip_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def coefficients(self):
        """hc as decod_init leaves it (the first ncols2convert columns in natural representation)."""
        out = np.empty((self.rh, self.nh), dtype=np.int16)
        _check(self.lib, self.lib.ldpc_hip_gfq_coefficients(self.h, out.ctypes.data), "ldpc_hip_gfq_coefficients")
        return out

    def decode(self, soft, maxiter, p_thr=0.0, want_qhard=True, want_post=False, stream=None):
        """soft: torch float64 CUDA tensor [B, q, N] (not modified).  Returns (qhard int16 [B, N] | None, iters int32 [B],
        post float64 [B, q, N] | None)."""
        import torch
        assert soft.is_cuda and soft.dtype == torch.float64 and soft.is_contiguous() and tuple(soft.shape[1:]) == (self.q, self.N)
        B = soft.shape[0]
        qhard = torch.empty((B, self.N), dtype=torch.int16, device=soft.device) if want_qhard else None
        iters = torch.empty((B,), dtype=torch.int32, device=soft.device)
        post = torch.empty((B, self.q, self.N), dtype=torch.float64, device=soft.device) if want_post else None
        rc = self.lib.ldpc_hip_decode_gfq_dev(self.h, soft.data_ptr(), B, int(maxiter), float(p_thr), qhard.data_ptr() if qhard is not None else None,
                                              iters.data_ptr(), post.data_ptr() if post is not None else None, _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_decode_gfq_dev")
        return qhard, iters, post

    def decode_host(self, soft, maxiter, p_thr=0.0, want_post=True):
        """soft: numpy float64 [B, q, N], laid out per frame like upstream's qy (not modified).  Returns (qhard int16 [B, N],
        iters int32 [B], post float64 [B, q, N] | None)."""
        soft = np.ascontiguousarray(soft, dtype=np.float64)
        if soft.ndim == 2:
            soft = soft[None]
        assert soft.shape[1:] == (self.q, self.N)
        B = soft.shape[0]
        qhard = np.empty((B, self.N), dtype=np.int16)
        iters = np.empty(B, dtype=np.int32)
        post = np.empty_like(soft) if want_post else None
        rc = self.lib.ldpc_hip_decode_gfq_host(self.h, soft.ctypes.data, B, int(maxiter), float(p_thr), qhard.ctypes.data, iters.ctypes.data,
                                               post.ctypes.data if post is not None else None)
        _check(self.lib, rc, "ldpc_hip_decode_gfq_host")
        return qhard, iters, post

    # ---- transmit side: encoder, q-ary channel, symbol-error counts, the chain ---------------------------------------------------
    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _to_dev(self, x, dtype, shape_tail, what):
        """torch CUDA tensor or numpy array -> (contiguous CUDA tensor [B, *shape_tail], was_numpy)."""
        import torch
        was_numpy = not isinstance(x, torch.Tensor)
        t = torch.from_numpy(np.ascontiguousarray(x)).to(self._dev()) if was_numpy else x
        if t.dim() == len(shape_tail):
            t = t[None]
        if not t.is_cuda or tuple(t.shape[1:]) != tuple(shape_tail):
            raise ValueError(f"{what}: expected a CUDA tensor or numpy array of shape [B, {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
        return t.to(dtype).contiguous(), was_numpy

    def sigma(self, snr_db):
        """bp_simulation.cpp:444-445 with punctured_blocks = 0."""
        return self.lib.ldpc_hip_gfq_sigma(self.h, float(snr_db))

    def encode(self, msg, stream=None):
        """msg [B, k] symbols 0 .. q-1 (torch CUDA tensor or numpy array; host arrays are checked).  Returns (codeword int16 [B, N],
        ok int32 [B]) -- encode_NBQCLDPC's codeword and return value per frame -- of the kind that was passed in."""
        import torch
        if not isinstance(msg, torch.Tensor):
            m = np.asarray(msg)
            if m.size and (m.min() < 0 or m.max() >= self.q):
                raise ValueError(f"encode: message symbols must lie in 0 .. {self.q - 1}")
        if self.k <= 0:   # nh <= rh: let the library name the rule
            _check(self.lib, self.lib.ldpc_hip_encode_gfq_dev(self.h, None, 0, None, None, None), "ldpc_hip_encode_gfq_dev")
        t, was_numpy = self._to_dev(msg, torch.int16, (self.k,), "encode")
        B = t.shape[0]
        cw = torch.empty((B, self.N), dtype=torch.int16, device=t.device)
        ok = torch.empty((B,), dtype=torch.int32, device=t.device)
        rc = self.lib.ldpc_hip_encode_gfq_dev(self.h, t.data_ptr(), B, cw.data_ptr(), ok.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_encode_gfq_dev")
        return (cw.cpu().numpy(), ok.cpu().numpy()) if was_numpy else (cw, ok)

    def channel(self, codeword=None, noise=None, sigma=None, seed=0, first_frame=0, B=None, stream=None):
        """Symbol probabilities [B, q, N] (torch CUDA float64) after BPSK + AWGN.  codeword [B, N] or None = the all-zero word; noise
        [B, N * q_bits] Gaussians or None = drawn on the device, keyed by (seed, first_frame + f, bit)."""
        import torch
        assert sigma is not None, "channel: sigma is required (see LdpcHipGfq.sigma)"
        cw = nz = None
        if codeword is not None:
            cw, _ = self._to_dev(codeword, torch.int16, (self.N,), "channel codeword")
            B = cw.shape[0] if B is None else B
        if noise is not None:
            nz, _ = self._to_dev(noise, torch.float64, (self.N * self.q_bits,), "channel noise")
            B = nz.shape[0] if B is None else B
        assert B is not None, "channel: B is required when neither codeword nor noise is given"
        if (cw is not None and cw.shape[0] != B) or (nz is not None and nz.shape[0] != B):
            raise ValueError("channel: codeword, noise and B disagree on the batch")
        soft = torch.empty((B, self.q, self.N), dtype=torch.float64, device=self._dev())
        rc = self.lib.ldpc_hip_gfq_channel_dev(self.h, cw.data_ptr() if cw is not None else None, nz.data_ptr() if nz is not None else None,
                                               float(sigma), int(seed), int(first_frame), int(B), soft.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_gfq_channel_dev")
        return soft

    def count_errors(self, qhard, codeword, iters, counters=None, stream=None):
        """qhard [B, N], codeword [B, N] or None = zero, iters [B].  Returns (counters uint64-valued int64 CUDA tensor [5] = nse, nde,
        nue, frames, sum |iters| -- `counters` itself, accumulated, when one is passed -- and frame_info int32 [B])."""
        import torch
        qh, _ = self._to_dev(qhard, torch.int16, (self.N,), "count_errors qhard")
        B = qh.shape[0]
        cw = None
        if codeword is not None:
            cw, _ = self._to_dev(codeword, torch.int16, (self.N,), "count_errors codeword")
        it = iters if isinstance(iters, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(iters)).to(self._dev())
        it = it.reshape(-1).to(torch.int32).contiguous()
        if it.shape[0] != B or (cw is not None and cw.shape[0] != B):
            raise ValueError("count_errors: qhard, codeword and iters disagree on the batch")
        if counters is None:
            counters = torch.zeros(5, dtype=torch.int64, device=self._dev())
        assert counters.is_cuda and counters.dtype == torch.int64 and counters.numel() == 5 and counters.is_contiguous()
        info = torch.empty((B,), dtype=torch.int32, device=self._dev())
        rc = self.lib.ldpc_hip_count_errors_gfq_dev(self.h, qh.data_ptr(), cw.data_ptr() if cw is not None else None, it.data_ptr(), B,
                                                    counters.data_ptr(), info.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_count_errors_gfq_dev")
        return counters, info

    def simulate(self, snr_db, maxiter, B, seed, first_frame=0, random_messages=True):
        """Frames [first_frame, first_frame + B) through encode -> channel -> decode -> count on the device.  Returns the five counters
        (nse, nde, nue, frames, sum |iters|) as Python ints."""
        cnt = (C.c_ulonglong * 5)()
        rc = self.lib.ldpc_hip_simulate_gfq(self.h, float(snr_db), int(maxiter), int(seed), int(first_frame), int(B), 1 if random_messages else 0, cnt)
        _check(self.lib, rc, "ldpc_hip_simulate_gfq")
        return [int(v) for v in cnt]

    # ---- exact replay of upstream's q-ary frame loop: its own mt19937 / normal_distribution stream, one word for all frames ----------
    def set_codeword(self, codeword=None):
        """The word every frame of mt_frames / frames_from_noise carries: [N] symbols 0 .. q-1, or None = the all-zero word."""
        cw = None
        if codeword is not None:
            cw = np.ascontiguousarray(codeword, dtype=np.int16)
            assert cw.shape == (self.N,)
        _check(self.lib, self.lib.ldpc_hip_gfq_set_codeword(self.h, cw.ctypes.data if cw is not None else None), "ldpc_hip_gfq_set_codeword")

    def mt_set_state(self, state, pos):
        """state: 624 uint32 words + index of the next word, as libstdc++ streams a std::mt19937."""
        st = np.ascontiguousarray(state, dtype=np.uint32)
        assert st.shape == (624,)
        _check(self.lib, self.lib.ldpc_hip_mt_set_state_gfq(self.h, st.ctypes.data, int(pos)), "ldpc_hip_mt_set_state_gfq")

    def mt_get_state(self):
        st = np.empty(624, dtype=np.uint32)
        pos = C.c_int()
        _check(self.lib, self.lib.ldpc_hip_mt_get_state_gfq(self.h, st.ctypes.data, C.byref(pos)), "ldpc_hip_mt_get_state_gfq")
        return st, pos.value

    def mt_advance(self, frames):
        """Draws and drops the frames * N * q_bits samples of `frames` frames."""
        _check(self.lib, self.lib.ldpc_hip_mt_advance_gfq(self.h, int(frames)), "ldpc_hip_mt_advance_gfq")

    def mt_frames(self, snr_db, maxiter, B, punctured_blocks=0):
        """noise -> channel -> decode -> count for the next B frames of upstream's stream: (frame_info, iters) int32 numpy arrays."""
        info = np.empty(max(int(B), 0), dtype=np.int32)
        its = np.empty(max(int(B), 0), dtype=np.int32)
        rc = self.lib.ldpc_hip_mt_frames_gfq(self.h, float(snr_db), int(punctured_blocks), int(maxiter), int(B), info.ctypes.data, its.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_frames_gfq")
        return info, its

    def frames_from_noise(self, noise, snr_db, maxiter, punctured_blocks=0):
        """The same records from Gaussians the caller drew: noise float64 numpy [B, N * q_bits] in upstream's order."""
        nz = np.ascontiguousarray(noise, dtype=np.float64)
        assert nz.ndim == 2 and nz.shape[1] == self.N * self.q_bits
        B = nz.shape[0]
        info = np.empty(B, dtype=np.int32)
        its = np.empty(B, dtype=np.int32)
        rc = self.lib.ldpc_hip_frames_gfq_noise_host(self.h, nz.ctypes.data, float(snr_db), int(punctured_blocks), int(maxiter), B,
                                                     info.ctypes.data, its.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_frames_gfq_noise_host")
        return info, its

    def profile(self, enable=True):
        _check(self.lib, self.lib.ldpc_hip_profile_enable(self.h, int(enable)), "ldpc_hip_profile_enable")

    def profile_read(self, reset=True):
        """(total milliseconds, launches) of the decode launches timed with HIP events since the last reset."""
        ms, n = C.c_double(), C.c_longlong()
        _check(self.lib, self.lib.ldpc_hip_profile_read(self.h, C.byref(ms), C.byref(n), int(reset)), "ldpc_hip_profile_read")
        return ms.value, n.value


def _code_stack(codes):
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    if codes.ndim == 2:
        codes = codes[None]
    assert codes.ndim == 3, "codes: [C, rh, nh] base matrices of one shape"
    return codes


# The entry points of a code set by decoder id: (open, whether it takes the id as its first argument, table, whether that one does).
# Any other id goes to the generic pair, which refuses it.
_CODES_GENERIC = ("ldpc_hip_open_codes", True, "ldpc_hip_codes_table_host", True)
_CODES_ROUTE = {
    DEC_SP: ("ldpc_hip_open_codes_sp", True, "ldpc_hip_codes_table_sp_host", True),
    DEC_ASP: ("ldpc_hip_open_codes_sp", True, "ldpc_hip_codes_table_sp_host", True),
    DEC_IMS: ("ldpc_hip_open_codes_ims", False, "ldpc_hip_codes_table_ims_host", False),
    DEC_IASP: ("ldpc_hip_open_codes_iasp", False, "ldpc_hip_codes_table_host", True),
    DEC_TASP: ("ldpc_hip_open_codes_tdmp", False, "ldpc_hip_codes_table_host", True),
    DEC_LCHE: ("ldpc_hip_open_codes_lche", False, "ldpc_hip_codes_table_lche_host", False),
}
# DEC_MS, DEC_TASP and DEC_LMS beyond the block rows (and, for DEC_MS, block columns) that their register-resident set kernels hold
_CODES_WIDE = ("ldpc_hip_open_codes_wide", True, "ldpc_hip_codes_table_wide_host", True)
# any shape: the global-memory tier of a set (csrc/ldpc_codeset_global.hpp), all eight set decoders
_CODES_GLOBAL = ("ldpc_hip_open_codes_global", True, "ldpc_hip_codes_table_global_host", True)
_EUNSUPPORTED = -2


def _codes_route(decoder_id, rh, nh):
    """The entry points that serve a set of rh x nh codes: the decoder's own where the shape fits them, the wide ones for DEC_MS,
    DEC_TASP and DEC_LMS exactly when rh > 16, or nh > 32 for DEC_MS."""
    if decoder_id in (DEC_MS, DEC_TASP, DEC_LMS) and (rh > 16 or (decoder_id == DEC_MS and nh > 32)):
        return _CODES_WIDE
    return _CODES_ROUTE.get(decoder_id, _CODES_GENERIC)


def _codes_entry(decoder_id, rh, nh, M, wide, tier):
    """The entry points a set opens through.  tier="global": the global-memory tier on any shape; tier="auto": that tier for M > 512
    (no other set kernel takes such a lifting), else wide=True or _codes_route.  wide=True keeps its entry point at any lifting (it
    refuses M > 512 as it always did); with tier="global" wide is ignored: the global tier has no wide variant."""
    if tier not in ("auto", "global"):
        raise ValueError(f'tier = {tier!r}: "auto" or "global"')
    if tier == "global" or (M > 512 and not wide):
        return _CODES_GLOBAL
    return _CODES_WIDE if wide else _codes_route(decoder_id, rh, nh)


def codes_table(decoder_id, codes, M, wide=False, tier="auto"):
    """The graph table of a code set as ldpc_hip_open_codes uploads it, built on the host (needs no GPU): (offsets int32 [C], table
    int32).  Code c owns table[offsets[c]:]: row_start[rh + 1], then its edges (block column << 16) | shift in row-major order; for
    DEC_IASP then cw2, col_start[nh + 1] and col_edges (edge index << 16) | shift in column-major order.  DEC_LCHE: the record of
    DEC_MS under LCHE's limits (ldpc_hip_codes_table_lche_host); DEC_IMS: the same record under integer min-sum's limits
    (ldpc_hip_codes_table_ims_host); DEC_SP, DEC_ASP: the record of DEC_IASP under the limits of the flooding sum-product set kernels
    (ldpc_hip_codes_table_sp_host).  DEC_MS, DEC_TASP and DEC_LMS beyond 16 block rows (DEC_MS: or 32 block columns): the record of
    DEC_MS under the limits of ldpc_hip_open_codes_wide (ldpc_hip_codes_table_wide_host); wide=True asks that entry point on any shape.
    tier="global", and tier="auto" for M > 512: the record of ldpc_hip_open_codes_global (ldpc_hip_codes_table_global_host) for all
    eight set decoders -- row_start[rh + 1], edges, cw2, col_start[nh + 1], col_edges (block row << 16) | shift and col_slot (the
    row-major index of the edge).  For M <= 512 tier="auto" answers for the decoder's own entry point, its refusal of an LDS image
    beyond 160 KiB included: the table of the set LdpcHipCodes then opens is the one of tier="global"."""
    lib = load_library()
    codes = _code_stack(codes)
    Cn, rh, nh = codes.shape
    n = C.c_longlong()
    _, _, who, takes_id = _codes_entry(int(decoder_id), rh, nh, int(M), wide, tier)
    head = (int(decoder_id),) if takes_id else ()
    call = lambda off, tab, cap, length: getattr(lib, who)(*head, rh, nh, int(M), codes.ctypes.data, Cn, off, tab, cap, length)
    _check(lib, call(None, None, 0, C.byref(n)), who)
    off = np.empty(Cn, dtype=np.int32)
    tab = np.empty(n.value, dtype=np.int32)
    _check(lib, call(off.ctypes.data, tab.ctypes.data, n.value, None), who)
    return off, tab


class LdpcHipCodes:
    """C candidate codes of one shape (codes int16 [C, rh, nh], lifting M) on one GPU, decoded C x B frames per launch (ldpc_hip_open_codes
    or the decoder's own open entry point, _CODES_ROUTE): what a code search scores.
    decoder_id DEC_MS, DEC_LMS, DEC_TASP, DEC_IASP, DEC_LCHE, DEC_IMS, DEC_SP or DEC_ASP; bit-identical to LdpcHip on each matrix.
    Block rows and columns are not limited: DEC_MS, DEC_TASP and DEC_LMS keep their register-resident kernels up to 16 block rows (DEC_MS:
    and 32 block columns) and open through ldpc_hip_open_codes_wide beyond (records in LDS); wide=True takes that route on any shape.
    No shape is refused: tier="auto" opens a lifting above 512 through ldpc_hip_open_codes_global (the state in a workspace in global
    memory), and any other set through the entry point above and, when that one answers LDPC_HIP_EUNSUPPORTED (an LDS image beyond
    160 KiB), through ldpc_hip_open_codes_global as well; a structural LDPC_HIP_EINVAL is raised under the first entry point's name.
    tier="global" takes that route on any shape (wide is ignored then).  self.entry names the entry point the set was opened through."""

    def __init__(self, decoder_id, codes, M, device=0, wide=False, tier="auto"):
        self.lib = load_library()
        codes = _code_stack(codes)
        self.C, self.rh, self.nh = codes.shape
        self.M, self.decoder_id, self.device = int(M), int(decoder_id), int(device)
        h = C.c_void_p()
        who, takes_id, _, _ = _codes_entry(self.decoder_id, self.rh, self.nh, self.M, wide, tier)
        head = (self.decoder_id,) if takes_id else ()
        rc = getattr(self.lib, who)(*head, self.rh, self.nh, self.M, codes.ctypes.data, self.C, self.device, C.byref(h))
        if rc == _EUNSUPPORTED and tier == "auto" and not wide and who != _CODES_GLOBAL[0]:   # the image does not fit the LDS
            who = _CODES_GLOBAL[0]
            rc = getattr(self.lib, who)(self.decoder_id, self.rh, self.nh, self.M, codes.ctypes.data, self.C, self.device, C.byref(h))
        _check(self.lib, rc, who)
        self.entry = who
        self.h = h
        self.N = self.lib.ldpc_hip_n(h)
        self.R = self.lib.ldpc_hip_r(h)
        self.hard_words = self.lib.ldpc_hip_hard_words(h)
        self.kernel_name = self.lib.ldpc_hip_kernel_name(h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldpc_hip_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def decode(self, llr, maxiter, alpha=0.8, shared=True, want_soft=False, stream=None):
        """llr: torch float64 CUDA tensor, [B, N] (shared=True: every code decodes the same received words) or [C, B, N].  Returns
        (hard int32 [C, B, W] -- the packed uint32 words --, iters int32 [C, B], soft float64 [C, B, N] | None)."""
        import torch
        assert llr.is_cuda and llr.dtype == torch.float64 and llr.is_contiguous()
        want = (self.N,) if shared else (self.C, None, self.N)
        assert llr.dim() == (2 if shared else 3) and llr.shape[-1] == self.N and (shared or llr.shape[0] == self.C), (tuple(llr.shape), want)
        B = llr.shape[-2]
        hard = torch.empty((self.C, B, self.hard_words), dtype=torch.int32, device=llr.device)
        iters = torch.empty((self.C, B), dtype=torch.int32, device=llr.device)
        soft = torch.empty((self.C, B, self.N), dtype=torch.float64, device=llr.device) if want_soft else None
        rc = self.lib.ldpc_hip_decode_codes_dev(self.h, llr.data_ptr(), 1 if shared else 0, B, int(maxiter), float(alpha), hard.data_ptr(),
                                                iters.data_ptr(), soft.data_ptr() if soft is not None else None, _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_decode_codes_dev")
        return hard, iters, soft

    def count_errors(self, hard, iters, counters=None, want_frame_info=False, stream=None):
        """hard [C, B, W], iters [C, B] as decode() returns them.  Returns (counters int64 CUDA tensor [C, 5] = nse, nde, nue, frames,
        sum |iters| per code -- `counters` itself, accumulated, when one is passed --, frame_info int32 [C, B] | None)."""
        import torch
        assert tuple(iters.shape[:1]) == (self.C,) and hard.is_contiguous() and iters.is_contiguous()
        B = iters.shape[1]
        if counters is None:
            counters = torch.zeros((self.C, 5), dtype=torch.int64, device=iters.device)
        assert counters.is_cuda and counters.dtype == torch.int64 and tuple(counters.shape) == (self.C, 5) and counters.is_contiguous()
        info = torch.empty((self.C, B), dtype=torch.int32, device=iters.device) if want_frame_info else None
        rc = self.lib.ldpc_hip_count_errors_codes_dev(self.h, hard.data_ptr(), iters.data_ptr(), B, info.data_ptr() if info is not None else None,
                                                      counters.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_count_errors_codes_dev")
        return counters, info

    def simulate(self, snr_db, maxiter, seed, first_frame, frames, punctured_blocks=0, alpha=0.8, records=False):
        """Frames [first_frame, first_frame + frames) of every code over the same noise.  Returns counters uint64 [C, 5] (nse, nde, nue,
        frames, sum |iters| per code: what LdpcHip.simulate gives for that matrix alone), and with records=True also frame_info
        int32 [C, frames]."""
        cnt = np.zeros((self.C, 5), dtype=np.uint64)
        info = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_simulate_codes(self.h, float(snr_db), int(punctured_blocks), int(maxiter), float(alpha), int(seed), int(first_frame),
                                              int(frames), cnt.ctypes.data, info.ctypes.data if info is not None else None)
        _check(self.lib, rc, "ldpc_hip_simulate_codes")
        return (cnt, info) if records else cnt

    def simulate_until(self, snr_db, maxiter, seed, n_frame_errors, n_experiments, reference_frame_error, first_frame=0, first_batch=1024,
                       max_batch=65536, punctured_blocks=0, alpha=0.8):
        """A Monte-Carlo run of every code over the same noise with upstream's stopping rule applied per code on the device
        (ldpc_hip_simulate_codes_stop): batches of first_batch frames, times 4 up to max_batch, each launch over the codes still
        running.  Returns uint64 [C, 4] = experiment, nse, nde, frames_decoded per code; the first three are what
        host.replay_stop_rule gives on the code's ordered records, frames_decoded counts the frames launched for it."""
        state = np.zeros((self.C, 4), dtype=np.uint64)
        rc = self.lib.ldpc_hip_simulate_codes_stop(self.h, float(snr_db), int(punctured_blocks), int(maxiter), float(alpha), int(seed), int(first_frame),
                                                   int(n_frame_errors), int(n_experiments), float(reference_frame_error), int(first_batch),
                                                   int(max_batch), state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_simulate_codes_stop")
        return state

    # ---- exact replay: upstream's own mt19937 / normal_distribution stream, drawn once per piece and shared by the codes ----------
    def mt_set_state(self, state, pos):
        """state: 624 uint32 words + index of the next word, as LdpcHip.mt_set_state."""
        st = np.ascontiguousarray(state, dtype=np.uint32)
        assert st.shape == (624,)
        _check(self.lib, self.lib.ldpc_hip_mt_set_state_codes(self.h, st.ctypes.data, int(pos)), "ldpc_hip_mt_set_state_codes")

    def mt_get_state(self):
        st = np.empty(624, dtype=np.uint32)
        pos = C.c_int()
        _check(self.lib, self.lib.ldpc_hip_mt_get_state_codes(self.h, st.ctypes.data, C.byref(pos)), "ldpc_hip_mt_get_state_codes")
        return st, pos.value

    def mt_advance(self, snr_db, frames, punctured_blocks=0):
        """Draws the next `frames` frames of the stream and drops them."""
        _check(self.lib, self.lib.ldpc_hip_mt_advance_codes(self.h, float(snr_db), int(punctured_blocks), int(frames)), "ldpc_hip_mt_advance_codes")

    def mt_simulate(self, snr_db, maxiter, frames, punctured_blocks=0, alpha=0.8, records=False):
        """The next `frames` frames of the stream for every code.  Returns counters uint64 [C, 5] (nse, nde, nue, frames, sum |iters| per
        code), and with records=True also frame_info and iters int32 [C, frames]: per code what LdpcHip.mt_frames gives for that matrix
        from the same generator state."""
        cnt = np.zeros((self.C, 5), dtype=np.uint64)
        info = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        its = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_mt_simulate_codes(self.h, float(snr_db), int(punctured_blocks), int(maxiter), float(alpha), int(frames), cnt.ctypes.data,
                                                 info.ctypes.data if records else None, its.ctypes.data if records else None)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes")
        return (cnt, info, its) if records else cnt

    def mt_simulate_until(self, snr_db, maxiter, n_frame_errors, n_experiments, reference_frame_error, first_batch=1024, max_batch=65536,
                          punctured_blocks=0, alpha=0.8):
        """simulate_until over the exact-replay stream (ldpc_hip_mt_simulate_codes_stop).  Returns uint64 [C, 6] = experiment, nse, nde,
        nue, sum |iters|, frames_decoded per code: upstream's SimCounters for that matrix after reset_random().  The generator is back
        at its state at entry afterwards; mt_advance(snr_db, state[c, 0]) takes it to the end of code c's run."""
        state = np.zeros((self.C, 6), dtype=np.uint64)
        rc = self.lib.ldpc_hip_mt_simulate_codes_stop(self.h, float(snr_db), int(punctured_blocks), int(maxiter), float(alpha), int(n_frame_errors),
                                                      int(n_experiments), float(reference_frame_error), int(first_batch), int(max_batch),
                                                      state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes_stop")
        return state

    # ---- an SNR grid: P points x C codes as P * C work items over one noise draw (ldpc_hip_*_codes_grid) ---------------
    @staticmethod
    def _points(snr_db):
        pts = np.ascontiguousarray(np.atleast_1d(snr_db), dtype=np.float64)
        assert pts.ndim == 1
        return pts

    def simulate_grid(self, snr_db, maxiter, seed, first_frame, frames, punctured_blocks=0, alpha=0.8, records=False):
        """simulate at every point of snr_db [P] (1 <= P <= 64) over one noise draw.  Returns counters uint64 [P, C, 5], and with
        records=True also frame_info int32 [P, C, frames]: row p is what simulate(snr_db[p], ...) returns."""
        pts = self._points(snr_db)
        P = len(pts)
        cnt = np.zeros((P, self.C, 5), dtype=np.uint64)
        info = np.empty((P, self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_simulate_codes_grid(self.h, pts.ctypes.data, P, int(punctured_blocks), int(maxiter), float(alpha), int(seed),
                                                   int(first_frame), int(frames), cnt.ctypes.data, info.ctypes.data if records else None)
        _check(self.lib, rc, "ldpc_hip_simulate_codes_grid")
        return (cnt, info) if records else cnt

    def simulate_grid_until(self, snr_db, maxiter, seed, n_frame_errors, n_experiments, reference_frame_error, first_frame=0, first_batch=1024,
                            max_batch=65536, punctured_blocks=0, alpha=0.8):
        """simulate_until at every point of snr_db [P] with reference_frame_error [P], the P * C items in one launch per piece.  Returns
        uint64 [P, C, 4]: row p is what simulate_until(snr_db[p], ..., reference_frame_error[p]) returns."""
        pts = self._points(snr_db)
        ref = np.ascontiguousarray(np.atleast_1d(reference_frame_error), dtype=np.float64)
        assert ref.shape == pts.shape
        state = np.zeros((len(pts), self.C, 4), dtype=np.uint64)
        rc = self.lib.ldpc_hip_simulate_codes_grid_stop(self.h, pts.ctypes.data, len(pts), int(punctured_blocks), int(maxiter), float(alpha), int(seed),
                                                        int(first_frame), int(n_frame_errors), int(n_experiments), ref.ctypes.data, int(first_batch),
                                                        int(max_batch), state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_simulate_codes_grid_stop")
        return state

    def mt_simulate_grid(self, snr_db, maxiter, frames, punctured_blocks=0, alpha=0.8, records=False):
        """mt_simulate at every point of snr_db [P] over the next `frames` frames of the stream, drawn once.  Returns counters uint64
        [P, C, 5], and with records=True also frame_info and iters int32 [P, C, frames]: row p is what mt_simulate(snr_db[p], ...) returns
        from the same generator state.  The generator is `frames` frames further on afterwards, once."""
        pts = self._points(snr_db)
        P = len(pts)
        cnt = np.zeros((P, self.C, 5), dtype=np.uint64)
        info = np.empty((P, self.C, int(frames)), dtype=np.int32) if records else None
        its = np.empty((P, self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_mt_simulate_codes_grid(self.h, pts.ctypes.data, P, int(punctured_blocks), int(maxiter), float(alpha), int(frames),
                                                      cnt.ctypes.data, info.ctypes.data if records else None, its.ctypes.data if records else None)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes_grid")
        return (cnt, info, its) if records else cnt

    def mt_simulate_grid_until(self, snr_db, maxiter, n_frame_errors, n_experiments, reference_frame_error, first_batch=1024, max_batch=65536,
                               punctured_blocks=0, alpha=0.8):
        """mt_simulate_until at every point of snr_db [P] with reference_frame_error [P].  Returns uint64 [P, C, 6]: row p is what
        mt_simulate_until(snr_db[p], ..., reference_frame_error[p]) returns.  The generator is back at its state at entry afterwards;
        mt_advance(snr_db[p], state[p, c, 0]) takes it to the end of item (p, c)."""
        pts = self._points(snr_db)
        ref = np.ascontiguousarray(np.atleast_1d(reference_frame_error), dtype=np.float64)
        assert ref.shape == pts.shape
        state = np.zeros((len(pts), self.C, 6), dtype=np.uint64)
        rc = self.lib.ldpc_hip_mt_simulate_codes_grid_stop(self.h, pts.ctypes.data, len(pts), int(punctured_blocks), int(maxiter), float(alpha),
                                                           int(n_frame_errors), int(n_experiments), ref.ctypes.data, int(first_batch), int(max_batch),
                                                           state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes_grid_stop")
        return state

    def set_ims_params(self, thr=1.4, qbits=6, dbits=8):
        """A DEC_IMS set: the quantiser arguments of imin_sum_decod_qc_lm for the next call (defaults MS_THR, MS_QBITS, MS_DBITS of
        decoders.h:46-48), as LdpcHip.set_ims_params."""
        _check(self.lib, self.lib.ldpc_hip_set_ims_params(self.h, float(thr), int(qbits), int(dbits)), "ldpc_hip_set_ims_params")

    def profile(self, enable=True):
        _check(self.lib, self.lib.ldpc_hip_profile_enable(self.h, int(enable)), "ldpc_hip_profile_enable")

    def profile_read(self, reset=True):
        """(total milliseconds, launches) of the decode launches timed with HIP events since the last reset."""
        ms, n = C.c_double(), C.c_longlong()
        _check(self.lib, self.lib.ldpc_hip_profile_read(self.h, C.byref(ms), C.byref(n), int(reset)), "ldpc_hip_profile_read")
        return ms.value, n.value


def _gfq_code_stacks(codes_hb, codes_hc):
    hb, hc = _code_stack(codes_hb), _code_stack(codes_hc)
    assert hb.shape == hc.shape, "codes_hb and codes_hc: [C, rh, nh] shifts and coefficients of the same codes"
    return hb, hc


def codes_gfq_table(q_bits, codes_hb, codes_hc, M):
    """The table of a GF(q) code set as ldpc_hip_open_codes_gfq uploads it, built on the host (needs no GPU): (offsets int32 [C], table
    int32).  Code c owns the record table[offsets[c]:] = E, cw2, row_start[rh + 1], col_start[nh + 1], e_col[E], e_circ[E], e_rl[E]
    (coefficient - 1), ce_edge[E]."""
    lib = load_library()
    hb, hc = _gfq_code_stacks(codes_hb, codes_hc)
    Cn, rh, nh = hb.shape
    n = C.c_longlong()
    _check(lib, lib.ldpc_hip_codes_gfq_table_host(int(q_bits), rh, nh, int(M), hb.ctypes.data, hc.ctypes.data, Cn, None, None, 0, C.byref(n)),
           "ldpc_hip_codes_gfq_table_host")
    off = np.empty(Cn, dtype=np.int32)
    tab = np.empty(n.value, dtype=np.int32)
    _check(lib, lib.ldpc_hip_codes_gfq_table_host(int(q_bits), rh, nh, int(M), hb.ctypes.data, hc.ctypes.data, Cn, off.ctypes.data, tab.ctypes.data,
                                                  n.value, None), "ldpc_hip_codes_gfq_table_host")
    return off, tab


class LdpcHipCodesGfq:
    """C candidate codes over GF(q), q = 2^q_bits, of one shape (codes_hb, codes_hc int16 [C, rh, nh]: shifts and coefficients as
    LdpcHipGfq takes them, lifting M) on one GPU, decoded C x B frames per launch (ldpc_hip_open_codes_gfq): what upstream's ggp
    search scores.  Bit-identical to LdpcHipGfq on each pair of matrices."""

    def __init__(self, q_bits, codes_hb, codes_hc, M, device=0):
        self.lib = load_library()
        hb, hc = _gfq_code_stacks(codes_hb, codes_hc)
        self.C, self.rh, self.nh = hb.shape
        self.M, self.q_bits, self.device = int(M), int(q_bits), int(device)
        h = C.c_void_p()
        rc = self.lib.ldpc_hip_open_codes_gfq(self.q_bits, self.rh, self.nh, self.M, hb.ctypes.data, hc.ctypes.data, self.C, self.device, C.byref(h))
        _check(self.lib, rc, "ldpc_hip_open_codes_gfq")
        self.h = h
        self.N = self.lib.ldpc_hip_n(h)
        self.R = self.lib.ldpc_hip_r(h)
        self.edges = self.lib.ldpc_hip_edges(h)
        self.q = self.lib.ldpc_hip_gfq_q(h)
        self.kernel_name = self.lib.ldpc_hip_kernel_name(h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldpc_hip_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sigma(self, snr_db):
        """bp_simulation.cpp:444-445 with punctured_blocks = 0: rh and nh only, common to the set."""
        return self.lib.ldpc_hip_gfq_sigma(self.h, float(snr_db))

    def decode(self, soft, maxiter, shared=True, want_post=False, stream=None):
        """soft: torch float64 CUDA tensor, [B, q, N] (shared=True: every code decodes the same received words) or [C, B, q, N]; not
        modified.  Returns (qhard int16 [C, B, N], iters int32 [C, B], post float64 [C, B, q, N] | None)."""
        import torch
        assert soft.is_cuda and soft.dtype == torch.float64 and soft.is_contiguous()
        assert soft.dim() == (3 if shared else 4) and tuple(soft.shape[-2:]) == (self.q, self.N) and (shared or soft.shape[0] == self.C), tuple(soft.shape)
        B = soft.shape[-3]
        qhard = torch.empty((self.C, B, self.N), dtype=torch.int16, device=soft.device)
        iters = torch.empty((self.C, B), dtype=torch.int32, device=soft.device)
        post = torch.empty((self.C, B, self.q, self.N), dtype=torch.float64, device=soft.device) if want_post else None
        rc = self.lib.ldpc_hip_decode_codes_gfq_dev(self.h, soft.data_ptr(), 1 if shared else 0, B, int(maxiter), qhard.data_ptr(), iters.data_ptr(),
                                                    post.data_ptr() if post is not None else None, _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_decode_codes_gfq_dev")
        return qhard, iters, post

    def count_errors(self, qhard, iters, counters=None, want_frame_info=False, stream=None):
        """qhard [C, B, N], iters [C, B] as decode() returns them, against the all-zero word.  Returns (counters int64 CUDA tensor
        [C, 5] = nse, nde, nue, frames, sum |iters| per code -- `counters` itself, accumulated, when one is passed --, frame_info int32
        [C, B] | None)."""
        import torch
        assert tuple(iters.shape[:1]) == (self.C,) and qhard.is_contiguous() and iters.is_contiguous()
        assert qhard.dtype == torch.int16 and iters.dtype == torch.int32 and tuple(qhard.shape) == (self.C, iters.shape[1], self.N)
        B = iters.shape[1]
        if counters is None:
            counters = torch.zeros((self.C, 5), dtype=torch.int64, device=iters.device)
        assert counters.is_cuda and counters.dtype == torch.int64 and tuple(counters.shape) == (self.C, 5) and counters.is_contiguous()
        info = torch.empty((self.C, B), dtype=torch.int32, device=iters.device) if want_frame_info else None
        rc = self.lib.ldpc_hip_count_errors_codes_gfq_dev(self.h, qhard.data_ptr(), iters.data_ptr(), B, info.data_ptr() if info is not None else None,
                                                          counters.data_ptr(), _stream_ptr(stream))
        _check(self.lib, rc, "ldpc_hip_count_errors_codes_gfq_dev")
        return counters, info

    def simulate(self, snr_db, maxiter, seed, first_frame, frames, records=False):
        """Frames [first_frame, first_frame + frames) of every code over the same noise, the all-zero word sent.  Returns counters
        uint64 [C, 5] (nse, nde, nue, frames, sum |iters| per code: what LdpcHipGfq.simulate(random_messages=False) gives for that
        code alone), and with records=True also frame_info int32 [C, frames]."""
        cnt = np.zeros((self.C, 5), dtype=np.uint64)
        info = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_simulate_codes_gfq(self.h, float(snr_db), int(maxiter), int(seed), int(first_frame), int(frames), cnt.ctypes.data,
                                                  info.ctypes.data if info is not None else None)
        _check(self.lib, rc, "ldpc_hip_simulate_codes_gfq")
        return (cnt, info) if records else cnt

    def simulate_until(self, snr_db, maxiter, seed, n_frame_errors, n_experiments, reference_frame_error, first_frame=0, first_batch=1024,
                       max_batch=65536):
        """LdpcHipCodes.simulate_until for a GF(q) set (ldpc_hip_simulate_codes_gfq_stop).  Returns uint64 [C, 4] = experiment, nse,
        nde, frames_decoded per code; nse counts wrong information symbols."""
        state = np.zeros((self.C, 4), dtype=np.uint64)
        rc = self.lib.ldpc_hip_simulate_codes_gfq_stop(self.h, float(snr_db), int(maxiter), int(seed), int(first_frame), int(n_frame_errors),
                                                       int(n_experiments), float(reference_frame_error), int(first_batch), int(max_batch), state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_simulate_codes_gfq_stop")
        return state

    # ---- exact replay of upstream's q-ary frame loop for every code of the set: one noise stream, a word per code -----------------------
    def set_codewords(self, words=None):
        """The word each code sends in mt_simulate / mt_simulate_until / frames_from_noise: [C, N] symbols 0 .. q-1, or None = every code
        sends the all-zero word and the soft values are shared."""
        w = None
        if words is not None:
            w = np.ascontiguousarray(words, dtype=np.int16)
            assert w.shape == (self.C, self.N)
        _check(self.lib, self.lib.ldpc_hip_codes_gfq_set_codewords(self.h, w.ctypes.data if w is not None else None), "ldpc_hip_codes_gfq_set_codewords")

    def mt_set_state(self, state, pos):
        st = np.ascontiguousarray(state, dtype=np.uint32)
        assert st.shape == (624,)
        _check(self.lib, self.lib.ldpc_hip_mt_set_state_codes_gfq(self.h, st.ctypes.data, int(pos)), "ldpc_hip_mt_set_state_codes_gfq")

    def mt_get_state(self):
        st = np.empty(624, dtype=np.uint32)
        pos = C.c_int()
        _check(self.lib, self.lib.ldpc_hip_mt_get_state_codes_gfq(self.h, st.ctypes.data, C.byref(pos)), "ldpc_hip_mt_get_state_codes_gfq")
        return st, pos.value

    def mt_advance(self, frames):
        """Draws and drops the frames * N * q_bits samples of `frames` frames."""
        _check(self.lib, self.lib.ldpc_hip_mt_advance_codes_gfq(self.h, int(frames)), "ldpc_hip_mt_advance_codes_gfq")

    def mt_simulate(self, snr_db, maxiter, frames, punctured_blocks=0, records=False):
        """The next `frames` frames of upstream's stream for every code.  Returns counters uint64 [C, 5], and with records=True also
        frame_info and iters int32 [C, frames]: per code what LdpcHipGfq.mt_frames gives for that code and word from the same state."""
        cnt = np.zeros((self.C, 5), dtype=np.uint64)
        info = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        its = np.empty((self.C, int(frames)), dtype=np.int32) if records else None
        rc = self.lib.ldpc_hip_mt_simulate_codes_gfq(self.h, float(snr_db), int(punctured_blocks), int(maxiter), int(frames), cnt.ctypes.data,
                                                     info.ctypes.data if records else None, its.ctypes.data if records else None)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes_gfq")
        return (cnt, info, its) if records else cnt

    def mt_simulate_until(self, snr_db, maxiter, n_frame_errors, n_experiments, reference_frame_error, first_batch=1024, max_batch=65536,
                          punctured_blocks=0):
        """Upstream's stopping rule per code over the exact-replay stream.  Returns uint64 [C, 6] = experiment, nse, nde, nue,
        sum |iters|, frames_decoded.  The generator is back at its state at entry afterwards; mt_advance(state[c, 0]) takes it to the
        end of code c's run."""
        state = np.zeros((self.C, 6), dtype=np.uint64)
        rc = self.lib.ldpc_hip_mt_simulate_codes_gfq_stop(self.h, float(snr_db), int(punctured_blocks), int(maxiter), int(n_frame_errors),
                                                          int(n_experiments), float(reference_frame_error), int(first_batch), int(max_batch),
                                                          state.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_simulate_codes_gfq_stop")
        return state

    def frames_from_noise(self, noise, snr_db, maxiter, punctured_blocks=0):
        """mt_simulate(records=True) from Gaussians the caller drew: noise float64 numpy [B, N * q_bits]."""
        nz = np.ascontiguousarray(noise, dtype=np.float64)
        assert nz.ndim == 2 and nz.shape[1] == self.N * self.q_bits
        B = nz.shape[0]
        cnt = np.zeros((self.C, 5), dtype=np.uint64)
        info = np.empty((self.C, B), dtype=np.int32)
        its = np.empty((self.C, B), dtype=np.int32)
        rc = self.lib.ldpc_hip_frames_codes_gfq_noise_host(self.h, nz.ctypes.data, float(snr_db), int(punctured_blocks), int(maxiter), B,
                                                           cnt.ctypes.data, info.ctypes.data, its.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_frames_codes_gfq_noise_host")
        return cnt, info, its

    def profile(self, enable=True):
        _check(self.lib, self.lib.ldpc_hip_profile_enable(self.h, int(enable)), "ldpc_hip_profile_enable")

    def profile_read(self, reset=True):
        """(total milliseconds, launches) of the decode launches timed with HIP events since the last reset."""
        ms, n = C.c_double(), C.c_longlong()
        _check(self.lib, self.lib.ldpc_hip_profile_read(self.h, C.byref(ms), C.byref(n), int(reset)), "ldpc_hip_profile_read")
        return ms.value, n.value


class LdpcHipMulti:
    """One opened code on several GPUs of a node behind the C-ABI (ldpc_hip_open_multi): one context + stream + host thread per
    shard, frames sharded by global frame index, the five counters all-reduced over RCCL (or summed on the host when shards
    share a device)."""

    def __init__(self, decoder_id, H, M, devices):
        self.lib = load_library()
        H = np.ascontiguousarray(H, dtype=np.int16)
        self.rh, self.nh = H.shape
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        rc = self.lib.ldpc_hip_open_multi(int(decoder_id), self.rh, self.nh, int(M), H.ctypes.data, devs.ctypes.data, len(devs), C.byref(h))
        _check(self.lib, rc, "ldpc_hip_open_multi")
        self.h = h
        self.N, self.R = self.nh * int(M), self.rh * int(M)
        self.shards = self.lib.ldpc_hip_multi_shards(h)
        self.reduction = self.lib.ldpc_hip_multi_reduction(h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ldpc_hip_close_multi(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_interleaver(self, permutation_type, permutation_block=128, permutation_inter=1):
        _check(self.lib, self.lib.ldpc_hip_multi_set_interleaver(self.h, int(permutation_type), int(permutation_block), int(permutation_inter)),
               "ldpc_hip_multi_set_interleaver")

    def set_codewords(self, codewords):
        if codewords is None or len(codewords) == 0:
            _check(self.lib, self.lib.ldpc_hip_multi_set_codewords(self.h, None, 0), "ldpc_hip_multi_set_codewords")
            return
        cw = np.ascontiguousarray(codewords, dtype=np.uint8).reshape(-1, self.N)
        _check(self.lib, self.lib.ldpc_hip_multi_set_codewords(self.h, cw.ctypes.data, cw.shape[0]), "ldpc_hip_multi_set_codewords")

    def simulate(self, snr_db, maxiter, seed, first_frame, B, batch, modulation=0, punctured_blocks=0, alpha=0.8, records=False):
        cnt = (C.c_ulonglong * 4)()
        sit = C.c_ulonglong()
        if records:
            info = np.empty(B, dtype=np.int32)
            its = np.empty(B, dtype=np.int32)
            rc = self.lib.ldpc_hip_frames_multi(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(maxiter), float(alpha),
                                                int(seed), int(first_frame), int(B), int(batch), info.ctypes.data, its.ctypes.data, cnt, C.byref(sit))
            _check(self.lib, rc, "ldpc_hip_frames_multi")
        else:
            info = its = None
            rc = self.lib.ldpc_hip_simulate_multi(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(maxiter), float(alpha),
                                                  int(seed), int(first_frame), int(B), int(batch), cnt, C.byref(sit))
            _check(self.lib, rc, "ldpc_hip_simulate_multi")
        out = {"nse": cnt[0], "nde": cnt[1], "nue": cnt[2], "frames": cnt[3], "sum_abs_iters": sit.value}
        if records:
            out["frame_info"], out["iters"] = info, its
        return out

    def ctx(self, shard):
        """Raw handle of shard i's context (per-shard settings and the single-device entry points)."""
        return C.c_void_p(self.lib.ldpc_hip_multi_ctx(self.h, int(shard)))

    def stream(self, shard):
        return C.c_void_p(self.lib.ldpc_hip_multi_stream(self.h, int(shard)))

    def channel_llr(self, shard, out, snr_db, seed, first_frame, modulation=0, punctured_blocks=0, T=26.0):
        """Fills `out` (float64 CUDA tensor [B, N] on the shard's device) with the decoder input of frames [first_frame, first_frame + B),
        on the shard's stream."""
        rc = self.lib.ldpc_hip_channel_llr_dev(self.ctx(shard), float(snr_db), int(modulation), int(punctured_blocks), float(T), int(seed),
                                               int(first_frame), int(out.shape[0]), C.c_void_p(out.data_ptr()), self.stream(shard))
        _check(self.lib, rc, "ldpc_hip_channel_llr_dev")
        return out

    def decode_count(self, batches, maxiter, first_frame=0, alpha=0.8):
        """The hot path on batches resident on the GPUs: batches[i] = float64 CUDA tensor [B, N] on shard i's device.  Returns the
        all-reduced counters."""
        assert len(batches) == self.shards
        B = int(batches[0].shape[0])
        ptrs = (C.c_void_p * self.shards)(*[C.c_void_p(b.data_ptr()) for b in batches])
        cnt = (C.c_ulonglong * 4)()
        sit = C.c_ulonglong()
        rc = self.lib.ldpc_hip_decode_count_multi(self.h, ptrs, B, int(first_frame), int(maxiter), float(alpha), cnt, C.byref(sit))
        _check(self.lib, rc, "ldpc_hip_decode_count_multi")
        return {"nse": cnt[0], "nde": cnt[1], "nue": cnt[2], "frames": cnt[3], "sum_abs_iters": sit.value}

    def mt_set_state(self, state, pos):
        st = np.ascontiguousarray(state, dtype=np.uint32)
        _check(self.lib, self.lib.ldpc_hip_mt_set_state_multi(self.h, st.ctypes.data, int(pos)), "ldpc_hip_mt_set_state_multi")

    def mt_get_state(self):
        st = np.empty(624, dtype=np.uint32)
        pos = C.c_int()
        _check(self.lib, self.lib.ldpc_hip_mt_get_state_multi(self.h, st.ctypes.data, C.byref(pos)), "ldpc_hip_mt_get_state_multi")
        return st, pos.value

    def mt_frames(self, snr_db, maxiter, B, modulation=0, punctured_blocks=0, alpha=0.8):
        info = np.empty(int(B), dtype=np.int32)
        its = np.empty(int(B), dtype=np.int32)
        rc = self.lib.ldpc_hip_mt_frames_multi(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(maxiter), float(alpha), int(B),
                                               info.ctypes.data, its.ctypes.data)
        _check(self.lib, rc, "ldpc_hip_mt_frames_multi")
        return info, its

    def mt_stats(self):
        """(generation rounds shared out over the shards, rounds redone with the whole tape on every shard)"""
        a, b = C.c_longlong(), C.c_longlong()
        self.lib.ldpc_hip_multi_mt_stats(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def mt_set_frame_index(self, frames_taken):
        _check(self.lib, self.lib.ldpc_hip_mt_set_frame_index_multi(self.h, int(frames_taken)), "ldpc_hip_mt_set_frame_index_multi")

    def mt_advance(self, snr_db, B, modulation=0, punctured_blocks=0):
        _check(self.lib, self.lib.ldpc_hip_mt_advance_multi(self.h, float(snr_db), int(modulation), int(punctured_blocks), int(B)), "ldpc_hip_mt_advance_multi")

    def decode_host(self, llr, maxiter, decision=0, alpha=0.8, clobber_sp_input=True):
        llr = np.array(llr, dtype=np.float64, order="C", copy=True)
        B = llr.shape[0]
        dec = np.empty((B, self.N), dtype=np.float64)
        its = np.empty(B, dtype=np.int32)
        rc = self.lib.ldpc_hip_decode_host_multi(self.h, llr.ctypes.data, B, int(maxiter), int(decision), float(alpha), dec.ctypes.data,
                                                 its.ctypes.data, 1 if clobber_sp_input else 0)
        _check(self.lib, rc, "ldpc_hip_decode_host_multi")
        return dec, its, llr


def mt_jump_host(state, log2_words):
    """mt19937 state 2**log2_words words further on (host, no GPU): the library's GF(2) polynomial jump."""
    lib = load_library()
    st = np.ascontiguousarray(state, dtype=np.uint32)
    out = np.empty(624, dtype=np.uint32)
    _check(lib, lib.ldpc_hip_mt_jump_host(st.ctypes.data, int(log2_words), out.ctypes.data), "ldpc_hip_mt_jump_host")
    return out


def girth_codes(hd, M, gmax=20, gtarget=4, min_ace=None, max_spec=None, device=0):
    """Upstream's trace_bound_pol_mon_pm on a set of codes [C, rh, nh] (or one code [rh, nh]) in one call (ldpc_hip_girth_codes):
    (S int32 [C, gmax], SA int32 [C, gmax], status int32 [C]; bit 0 = upstream's return value, bit 1 = a 32-bit sum overflowed).
    min_ace / max_spec: upstream's minSA / maxS, [gmax] each, or None."""
    lib = load_library()
    codes = _code_stack(hd)
    Cn, rh, nh = codes.shape
    gmax = int(gmax)
    rows = max(gmax, 0)
    bounds = [None if b is None else np.ascontiguousarray(b, dtype=np.int32) for b in (min_ace, max_spec)]
    for b in bounds:
        assert b is None or b.shape == (gmax,), "min_ace / max_spec: [gmax]"
    S = np.zeros((Cn, rows), dtype=np.int32)
    SA = np.zeros((Cn, rows), dtype=np.int32)
    status = np.zeros(Cn, dtype=np.int32)
    rc = lib.ldpc_hip_girth_codes(rh, nh, int(M), codes.ctypes.data, Cn, gmax, int(gtarget), *(None if b is None else b.ctypes.data for b in bounds),
                                  int(device), S.ctypes.data, SA.ctypes.data, status.ctypes.data)
    _check(lib, rc, "ldpc_hip_girth_codes")
    return S, SA, status


def girth_graph(hd, M):
    """The graph the girth kernels walk, built on the host (no GPU): (E, pred_begin int32 [E + 1], pred int32 [n, 3]) -- the
    predecessors (j, a, as) of edge J are pred[pred_begin[J]:pred_begin[J + 1]], j ascending."""
    lib = load_library()
    H = np.ascontiguousarray(hd, dtype=np.int16)
    rh, nh = H.shape
    E, n = C.c_int(), C.c_longlong()
    _check(lib, lib.ldpc_hip_girth_graph_host(rh, nh, int(M), H.ctypes.data, C.byref(E), None, None, C.byref(n)), "ldpc_hip_girth_graph_host")
    begin = np.empty(E.value + 1, dtype=np.int32)
    pred = np.empty((n.value, 3), dtype=np.int32)
    _check(lib, lib.ldpc_hip_girth_graph_host(rh, nh, int(M), H.ctypes.data, C.byref(E), begin.ctypes.data, pred.ctypes.data, C.byref(n)),
           "ldpc_hip_girth_graph_host")
    return E.value, begin, pred


def trace_matrix(S, SA):
    """main_simulation.cpp:177-201 on one code's S / SA (host, no GPU): (girth -- 21 when no cycle was found --, ACE [4], spectrum [4])."""
    lib = load_library()
    S = np.ascontiguousarray(S, dtype=np.int32)
    SA = np.ascontiguousarray(SA, dtype=np.int32)
    assert S.ndim == 1 and S.shape == SA.shape, "S, SA: [gmax] of one code"
    girth = C.c_int()
    ace = np.zeros(4, dtype=np.int32)
    spec = np.zeros(4, dtype=np.int32)
    _check(lib, lib.ldpc_hip_trace_matrix_host(S.ctypes.data, SA.ctypes.data, S.size, C.byref(girth), ace.ctypes.data, spec.ctypes.data),
           "ldpc_hip_trace_matrix_host")
    return girth.value, ace.tolist(), spec.tolist()


def label_equations(proto, target_girth):
    """The equations a labelling of the protograph [rh, nh] (0 empty, 1 random shift, other positive values shift 0) must satisfy to
    reach target_girth, built on the host (no GPU; ldpc_hip_label_equations_host): a dict with tree_girth, n_equations, n_random,
    never_accepts and the table eq_begin int32 [n_equations + 1], term_edge, term_mult int32 [n_terms] over the random edges."""
    lib = load_library()
    P = np.ascontiguousarray(proto, dtype=np.int16)
    rh, nh = P.shape
    tg, ne, nr, never, nt = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    sizes = (C.byref(tg), C.byref(ne), C.byref(nr), C.byref(nt), C.byref(never))
    _check(lib, lib.ldpc_hip_label_equations_host(rh, nh, P.ctypes.data, int(target_girth), *sizes, None, None, None), "ldpc_hip_label_equations_host")
    begin = np.empty(ne.value + 1, dtype=np.int32)
    edge = np.empty(nt.value, dtype=np.int32)
    mult = np.empty(nt.value, dtype=np.int32)
    _check(lib, lib.ldpc_hip_label_equations_host(rh, nh, P.ctypes.data, int(target_girth), *sizes, begin.ctypes.data, edge.ctypes.data, mult.ctypes.data),
           "ldpc_hip_label_equations_host")
    return {"tree_girth": tg.value, "n_equations": ne.value, "n_random": nr.value, "never_accepts": bool(never.value), "eq_begin": begin,
            "term_edge": edge, "term_mult": mult}


def label_codes(proto, target_girth, M, max_attempts, state, pos, want=1, device=0):
    """Upstream's generate_code on the device (ldpc_hip_label_codes): labels the protograph with shifts below M until `want` labellings
    pass the girth equations and the equal-columns test, or max_attempts are used up, drawing from the std::mt19937 (state uint32
    [624], pos).  Returns (codes int16 [found, rh, nh], attempt_index int64 [found] -- 0-based over the whole call --, attempts_tested,
    tree_girth, (state, pos) of the generator afterwards)."""
    lib = load_library()
    P = np.ascontiguousarray(proto, dtype=np.int16)
    rh, nh = P.shape
    st = np.ascontiguousarray(state, dtype=np.uint32)
    assert st.shape == (624,), "state: the 624 words of std::mt19937"
    want = int(want)
    codes = np.zeros((max(want, 0), rh, nh), dtype=np.int16)
    index = np.zeros(max(want, 0), dtype=np.int64)
    out = np.zeros(624, dtype=np.uint32)
    found, tg, pos_out, tested = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    rc = lib.ldpc_hip_label_codes(rh, nh, P.ctypes.data, int(target_girth), int(M), int(max_attempts), want, st.ctypes.data, int(pos), int(device),
                                  codes.ctypes.data, index.ctypes.data, C.byref(found), C.byref(tested), C.byref(tg), out.ctypes.data, C.byref(pos_out))
    _check(lib, rc, "ldpc_hip_label_codes")
    return codes[:found.value], index[:found.value], tested.value, tg.value, (out, pos_out.value)


def label_last_stats():
    """(rounds, redraws, equations evaluated by live lanes, attempts checked) of this thread's last label_codes."""
    s = np.zeros(4, dtype=np.int64)
    load_library().ldpc_hip_label_last_stats(s.ctypes.data)
    return tuple(int(v) for v in s)


def check_voltages(proto, target_girth, voltages, max_modulo, coefs=None, device=0):
    """Upstream's check_voltages (coefs=None) / check_voltages_and_coefs for a batch of labellings on the device
    (ldpc_hip_check_voltages): proto [rh, nh] (any positive entry is an edge), voltages and coefs int32 [K, E] or [E] in 0 .. 32767
    over the edges column by column.  Returns a dict: status, min_ok, max_nonok, max_abs_sum int32 [K], failed uint64
    [K, max_modulo // 64 + 1] (bit m: m is a failed modulo), tree_girth, n_equations.  status 0 = ok, 1 = an identically zero sum,
    2 = a zero sum rescued by its coefficients (upstream exits there)."""
    lib = load_library()
    P = np.ascontiguousarray(proto, dtype=np.int16)
    rh, nh = P.shape
    V = np.ascontiguousarray(np.atleast_2d(np.asarray(voltages)), dtype=np.int32)
    K = V.shape[0]
    Cf = None if coefs is None else np.ascontiguousarray(np.atleast_2d(np.asarray(coefs)), dtype=np.int32)
    assert V.ndim == 2 and V.shape[1] == int((P > 0).sum()), "voltages: [K, E], one per edge"
    assert Cf is None or Cf.shape == V.shape, "coefs: as voltages"
    W = int(max_modulo) // 64 + 1 if 1 <= int(max_modulo) <= 65535 else 1
    status, min_ok, max_nonok, max_abs = (np.zeros(K, dtype=np.int32) for _ in range(4))
    failed = np.zeros((K, W), dtype=np.uint64)
    tg, ne = C.c_int(), C.c_int()
    rc = lib.ldpc_hip_check_voltages(rh, nh, P.ctypes.data, int(target_girth), int(max_modulo), V.ctypes.data, None if Cf is None else Cf.ctypes.data, K,
                                     int(device), status.ctypes.data, min_ok.ctypes.data, max_nonok.ctypes.data, max_abs.ctypes.data, failed.ctypes.data,
                                     C.byref(tg), C.byref(ne))
    _check(lib, rc, "ldpc_hip_check_voltages")
    return {"status": status, "min_ok": min_ok, "max_nonok": max_nonok, "max_abs_sum": max_abs, "failed": failed, "tree_girth": tg.value,
            "n_equations": ne.value}


def failed_moduli(failed_row):
    """The members of one labelling's failed set, ascending, from its bitmap row of check_voltages."""
    bits = np.unpackbits(np.ascontiguousarray(failed_row, dtype="<u8").view(np.uint8), bitorder="little")
    return np.flatnonzero(bits)


def label_bank(proto, target_girth, T, max_attempts, state, pos, want=1, exact_modulo=0, device=0):
    """The loop of upstream's random_search_bank_good_codes with a budget (ldpc_hip_label_bank): as label_codes with shifts below the
    tailbite length T, an attempt being accepted when its voltage check is ok, its smallest lifting min_ok <= T and, with
    exact_modulo != 0, check_modulo(exact_modulo).  Returns (codes int16 [found, rh, nh], min_ok int32 [found], attempt_index int64
    [found], attempts_tested, tree_girth, (state, pos) of the generator afterwards)."""
    lib = load_library()
    P = np.ascontiguousarray(proto, dtype=np.int16)
    rh, nh = P.shape
    st = np.ascontiguousarray(state, dtype=np.uint32)
    assert st.shape == (624,), "state: the 624 words of std::mt19937"
    want = int(want)
    codes = np.zeros((max(want, 0), rh, nh), dtype=np.int16)
    min_ok = np.zeros(max(want, 0), dtype=np.int32)
    index = np.zeros(max(want, 0), dtype=np.int64)
    out = np.zeros(624, dtype=np.uint32)
    found, tg, pos_out, tested = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
    rc = lib.ldpc_hip_label_bank(rh, nh, P.ctypes.data, int(target_girth), int(T), int(exact_modulo), int(max_attempts), want, st.ctypes.data, int(pos),
                                 int(device), codes.ctypes.data, min_ok.ctypes.data, index.ctypes.data, C.byref(found), C.byref(tested), C.byref(tg),
                                 out.ctypes.data, C.byref(pos_out))
    _check(lib, rc, "ldpc_hip_label_bank")
    return codes[:found.value], min_ok[:found.value], index[:found.value], tested.value, tg.value, (out, pos_out.value)


def qam_modulate(bits, Q, device=0, stream=None):
    """Function-level mapper (QAM_modulator.cpp QAM_modulator): uint8 CUDA tensor bits[ns, log2 Q] -> float64 [ns, 2] (I, Q)."""
    import torch
    lib = load_library()
    ns = bits.shape[0]
    out = torch.empty((ns, 2), dtype=torch.float64, device=bits.device)
    rc = lib.ldpc_hip_qam_modulate_dev(int(Q), bits.data_ptr(), ns, out.data_ptr(), device, _stream_ptr(stream))
    _check(lib, rc, "ldpc_hip_qam_modulate_dev")
    return out


def encode(H, M, info_bits):
    """Systematic QC-LDPC encoding on the host (upstream's qc_encode / random_codeword with given information bits):
    info_bits uint8[(nh-rh)*M] -> codeword uint8[nh*M] (parity part first).  Needs no GPU."""
    lib = load_library()
    H = np.ascontiguousarray(H, dtype=np.int16)
    rh, nh = H.shape
    info = np.ascontiguousarray(info_bits, dtype=np.uint8)
    assert info.size == (nh - rh) * M
    cw = np.empty(nh * M, dtype=np.uint8)
    _check(lib, lib.ldpc_hip_encode_host(rh, nh, int(M), H.ctypes.data, info.ctypes.data, cw.ctypes.data), "ldpc_hip_encode_host")
    return cw


def build_interleaver(H, M, mode, halfmlog=1, block_size=128, step_size=1):
    """Gather maps (direct, inverse) of upstream's interleaver `mode` (permutation_type) for base matrix H: out[i] = in[map[i]].
    Host-side, needs no GPU."""
    lib = load_library()
    H = np.ascontiguousarray(H, dtype=np.int16)
    b, c = H.shape
    direct = np.empty(c * M, dtype=np.int32)
    inverse = np.empty(c * M, dtype=np.int32)
    rc = lib.ldpc_hip_interleaver_build(b, c, int(M), int(halfmlog), int(mode), int(block_size), int(step_size), H.ctypes.data,
                                        direct.ctypes.data, inverse.ctypes.data)
    _check(lib, rc, "ldpc_hip_interleaver_build")
    return direct, inverse


def permute(x, index_map, device=0, stream=None):
    """y[f, i] = x[f, index_map[i]] on the GPU (x float64 CUDA [B, N], index_map int32 CUDA [N])."""
    import torch
    lib = load_library()
    y = torch.empty_like(x)
    rc = lib.ldpc_hip_permute_dev(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], index_map.data_ptr(), device, _stream_ptr(stream))
    _check(lib, rc, "ldpc_hip_permute_dev")
    return y


def qam_demod(x, Q, T, sigma, out_type=0, device=0, stream=None):
    """Function-level soft demapper (QAM_demodulator.cpp Demodulate) on a CUDA float64 tensor x[ns,2] -> [ns, log2 Q]."""
    import torch
    lib = load_library()
    m = {4: 2, 16: 4, 64: 6, 256: 8}[Q]
    ns = x.shape[0]
    out = torch.empty((ns, m), dtype=torch.float64, device=x.device)
    rc = lib.ldpc_hip_qam_demod_dev(Q, float(T), float(sigma), x.data_ptr(), ns, out.data_ptr(), out_type, device, _stream_ptr(stream))
    _check(lib, rc, "ldpc_hip_qam_demod_dev")
    return out
