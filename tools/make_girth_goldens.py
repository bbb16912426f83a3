#!/usr/bin/env python3
"""Golden results of the girth / ACE trace from the COMPILED UPSTREAM REFERENCE: trace_bound_pol_mon_pm (trace_pm.cpp, NATURAL_POLYNOM).

Run where the upstream tree is mounted (REF, default as in oracle/Makefile):

    python3 tools/make_girth_goldens.py [case names...]

It compiles upstream's trace_pm.cpp and 3d_array.cpp unchanged, with the driver below, into oracle/_ref/girth_ref (never committed)
-- with -fsanitize=signed-integer-overflow, so a case on which upstream's 32-bit sums overflow aborts the run instead of being
recorded -- and writes one tests/golden/girth/<case>.json per case: the inputs (codes [C][rh][nh], M, gmax, gtarget, min_ace, max_spec)
and upstream's S, SA and return value per code.  Every case is also checked against the numpy restatement tests/girth_model.py,
whose int64 peak must stay below 2^31.  The cases, and what each is for, are listed in cases()."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import girth_model  # noqa: E402
from ldpc_testlib import load_base_matrix, relift  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
EXE = os.path.join(ROOT, "oracle", "_ref", "girth_ref")

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "trace_pm.h"
int main() {
    int rh, nh, M, gmax, gtarget, use_min, use_max;
    if (scanf("%d %d %d %d %d %d %d", &rh, &nh, &M, &gmax, &gtarget, &use_min, &use_max) != 7) return 2;
    std::vector<int> mn(gmax), mx(gmax), S(gmax), SA(gmax);
    for (int &v : mn) if (scanf("%d", &v) != 1) return 2;
    for (int &v : mx) if (scanf("%d", &v) != 1) return 2;
    ARRAY hd;
    hd.ndim = 2;
    put_nrow(&hd, rh);
    put_ncol(&hd, nh);
    put_addr(&hd, Alloc2d_int(rh, nh));
    for (int j = 0; j < rh; ++j)
        for (int k = 0; k < nh; ++k)
            if (scanf("%d", &hd.addr[j][k]) != 1) return 2;
    const int ret = trace_bound_pol_mon_pm(hd, M, gmax, gtarget, S.data(), SA.data(), use_min ? mn.data() : NULL, use_max ? mx.data() : NULL);
    for (int v : S) printf("%d ", v);
    printf("\n");
    for (int v : SA) printf("%d ", v);
    printf("\n%d\n", ret);
    return 0;
}
"""

PASS_MIN, PASS_MAX = [0] * 20, [100000000] * 20     # main_simulation.cpp:162-163: bounds every matrix passes

# the GF(16) code of upstream's files/resultq_codes.jsonx (4 x 8), shifts % 8
GF16 = np.array([[0, -1, -1, 73, 2, -1, -1, 1], [0, 0, -1, -1, -1, 11, -1, -1], [-1, 0, 0, -1, 1, -1, 13, 17], [-1, -1, 0, 12, -1, 13, 1, -1]])
SMALL = np.array([[0, 3, -1, 5, 1, -1], [2, -1, 4, 0, -1, 6], [-1, 1, 0, -1, 3, 2]])   # 3 x 6


def plain(H, M):
    H = np.array(H, dtype=np.int64)
    return np.where(H >= 0, H % M, -1)


def random_shifts(mask, M, rng, n):
    return np.stack([np.where(mask, rng.randint(0, M, mask.shape), -1) for _ in range(n)])


def appendix_c(M):
    return plain(load_base_matrix(), M)[None]


def sim_pair(M):
    """Two 16 x 32 codes as ldpc_sim reduces them (main_simulation.cpp:400-414): Appendix C and a variant with other shifts in the
    information columns."""
    H = load_base_matrix()
    other = H.copy()
    info = other[:, 16:]
    info[info >= 0] = (info[info >= 0] * 5 + 3) % 126
    return np.stack([relift(H, M), relift(other, M)])


def cases():
    """name -> (codes [C, rh, nh], M, gmax, gtarget, min_ace, max_spec)"""
    rng = np.random.RandomState(2028)
    gf16 = plain(GF16, 8)[None]
    small = plain(SMALL, 7)[None]
    out = {
        # lifting and the removal of the constant term: M = 126 is the case where upstream's way of removing it changes SA[11]
        "appc_m126": (appendix_c(126), 126, 20, 4, PASS_MIN, PASS_MAX),
        "appc_m64": (appendix_c(64), 64, 20, 4, PASS_MIN, PASS_MAX),            # a wave's multiple
        "appc_m67": (appendix_c(67), 67, 20, 4, PASS_MIN, PASS_MAX),            # no power of two, two waves
        "appc_m5": (appendix_c(5), 5, 20, 4, PASS_MIN, PASS_MAX),               # below a wave
        "appc_m1": (appendix_c(1), 1, 20, 4, PASS_MIN, PASS_MAX),
        "appc_m5_gtarget1": (appendix_c(5), 5, 20, 1, PASS_MIN, PASS_MAX),
        # what ldpc_sim traces: main_simulation.cpp:400-414 on the same matrix
        "sim_pair_m126": (sim_pair(126), 126, 20, 4, PASS_MIN, PASS_MAX),
        "sim_pair_m64": (sim_pair(64), 64, 20, 4, PASS_MIN, PASS_MAX),
        "small_m7": (small, 7, 20, 4, PASS_MIN, PASS_MAX),
        "small_m7_gmax8": (small, 7, 8, 4, PASS_MIN[:8], PASS_MAX[:8]),
        "gf16_m8": (gf16, 8, 20, 4, PASS_MIN, PASS_MAX),
        # rows longer than one workgroup's lanes (M > 1024), in LDS and -- beyond 160 KB per row -- in global memory
        "small_m1100": (plain(SMALL * 157, 1100)[None], 1100, 20, 4, PASS_MIN, PASS_MAX),
        "small_m2400": (plain(SMALL * 331, 2400)[None], 2400, 20, 4, PASS_MIN, PASS_MAX),
        # no cycle up to length 20: a path
        "no_cycle": (np.array([[[0, 1, -1, -1], [-1, 2, 3, -1], [-1, -1, 1, 0]]]), 5, 20, 4, PASS_MIN, PASS_MAX),
        # 4-cycles: all shifts equal
        "four_cycles": (np.zeros((1, 3, 4), dtype=np.int64), 3, 20, 4, PASS_MIN, PASS_MAX),
        # columns of weight 1 and an all-empty column
        "column_weights": (np.array([[[0, 2, -1, 1, -1, 3], [1, -1, -1, 0, 4, -1], [-1, 3, -1, 2, -1, -1]]]), 6, 20, 4, PASS_MIN, PASS_MAX),
    }
    # bounds on the GF(16) shape.  The rule divides as integers (S / (d + 1), SA / 2), so a bound of -1 on the spectrum and one of
    # 1000 on the ace fail whatever the entry is; entry `cnt` of a bound is read at the (cnt + 1)-th non-zero S[d]
    fail_first, fail_second = [-1] + [100000000] * 19, [100000000, -1] + [100000000] * 18
    ace_fail_second = [0, 1000] + [0] * 18
    out.update({
        "bounds_spec_fails_first": (gf16, 8, 20, 4, None, fail_first),
        "bounds_spec_fails_second": (gf16, 8, 20, 4, None, fail_second),
        "bounds_spec_only_passes": (gf16, 8, 20, 4, None, PASS_MAX),
        "bounds_ace_only_passes": (gf16, 8, 20, 4, PASS_MIN, None),
        "bounds_ace_fails_second": (gf16, 8, 20, 4, ace_fail_second, None),
        "bounds_either_passes_by_ace": (gf16, 8, 20, 4, PASS_MIN, [0] * 20),
        "bounds_either_passes_by_spec": (gf16, 8, 20, 4, [1000] * 20, PASS_MAX),
        "bounds_both_fail_second": (gf16, 8, 20, 4, ace_fail_second, fail_second),
        "bounds_neither": (gf16, 8, 20, 4, None, None),
    })
    # a set over one mask whose girths and stopping depths differ; a set with two masks (different E)
    one_mask = random_shifts(GF16 >= 0, 16, rng, 40)
    seen, pick = set(), []
    for c in one_mask:
        S, SA, ok, _ = girth_model.trace(c, 16, 20, 4, [7, 11, 0, 0] + [0] * 16, None)
        key = (girth_model.trace_matrix(S, SA)[0], int(np.flatnonzero(S).max()), ok)
        if key not in seen or len(pick) < 3:
            seen.add(key)
            pick.append(c)
        if len(pick) == 6:
            break
    assert len(seen) >= 3, seen
    out["set_one_mask"] = (np.stack(pick), 16, 20, 4, [7, 11, 0, 0] + [0] * 16, None)
    other = np.array([[1, 1, 0, 0, 1, 1, 0, 1], [1, 0, 1, 1, 0, 1, 1, 0], [0, 1, 1, 0, 1, 0, 1, 1], [1, 1, 0, 1, 1, 1, 0, 1]], dtype=bool)
    out["set_two_masks"] = (np.concatenate([random_shifts(GF16 >= 0, 9, rng, 2), random_shifts(other, 9, rng, 2)])[[0, 2, 1, 3]], 9, 20, 4,
                            PASS_MIN, PASS_MAX)
    return out


def build_reference():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(os.path.dirname(EXE), "girth_ref_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-O2", "-w", "-fsanitize=signed-integer-overflow", "-fno-sanitize-recover=all", "-I", REF, src,
                           os.path.join(REF, "trace_pm.cpp"), os.path.join(REF, "3d_array.cpp"), "-o", EXE])


def reference(hd, M, gmax, gtarget, min_ace, max_spec):
    words = [hd.shape[0], hd.shape[1], M, gmax, gtarget, int(min_ace is not None), int(max_spec is not None)]
    words += list(min_ace if min_ace is not None else [0] * gmax) + list(max_spec if max_spec is not None else [0] * gmax)
    words += [int(v) for v in hd.reshape(-1)]
    out = subprocess.run([EXE], input=" ".join(str(w) for w in words), capture_output=True, text=True, check=True).stdout.split("\n")
    return [int(v) for v in out[0].split()], [int(v) for v in out[1].split()], int(out[2])


def main(argv):
    assert os.path.isdir(REF), f"the upstream tree is not mounted at {REF}"
    build_reference()
    os.makedirs(girth_model.GIRTH_GOLDEN_DIR, exist_ok=True)
    for name, (codes, M, gmax, gtarget, min_ace, max_spec) in cases().items():
        if argv and name not in argv:
            continue
        codes = np.asarray(codes, dtype=np.int64)
        S, SA, ret, peaks = [], [], [], []
        for hd in codes:
            s, sa, r = reference(hd, M, gmax, gtarget, min_ace, max_spec)
            ms, msa, mr, peak = girth_model.trace(hd, M, gmax, gtarget, min_ace, max_spec)
            assert peak < 2 ** 31, f"{name}: peak {peak}"
            assert ms.tolist() == s and msa.tolist() == sa and mr == r, f"{name}: model != reference\n{ms.tolist()}\n{s}\n{msa.tolist()}\n{sa}\n{mr} {r}"
            S.append(s), SA.append(sa), ret.append(r), peaks.append(peak)
        path = os.path.join(girth_model.GIRTH_GOLDEN_DIR, name + ".json")
        with open(path, "w") as f:
            json.dump({"codes": codes.tolist(), "M": M, "gmax": gmax, "gtarget": gtarget, "min_ace": None if min_ace is None else list(min_ace),
                       "max_spec": None if max_spec is None else list(max_spec), "S": S, "SA": SA, "ret": ret}, f, separators=(",", ":"))
            f.write("\n")
        girths = [girth_model.trace_matrix(s, sa)[0] for s, sa in zip(S, SA)]
        print(f"{name}: C = {len(codes)}, girth {girths}, return {ret}, peak {max(peaks)}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
