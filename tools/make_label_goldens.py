#!/usr/bin/env python3
"""Golden results of the labelling search from the COMPILED UPSTREAM SOURCES: generate_code (code_generation.cpp) with its equation
builder (equations.cpp, graph_spider.h, data_structures.cpp, combinatorics.cpp).

Run where the upstream tree is mounted (REF, default as in oracle/Makefile):

    python3 tools/make_label_goldens.py [case names...]

It compiles those four upstream files unchanged, with the driver below, into oracle/_ref/label_ref (never committed).  The fifth file on
the path, commons_portable.cpp, does not compile against a current glibc (<stropts.h>, see oracle/Makefile), so the driver supplies the
few symbols of it that generate_code reaches -- as tests/cpp/dropin_driver.cpp does for bp_simulation: the global std::mt19937 seeded from
initial_random_seed, next_random_int as a fresh uniform_int_distribution<int> per call, and console hooks that do nothing.  The driver
sets the seed, calls generate_code K times in a row and then draws eight next_random_int(0, 1 << 30) as a fingerprint of the generator
(such a draw is the next word >> 2 and is never rejected).  One tests/golden/label/<case>.json per case: the inputs, per call ok /
attempts tested / result matrix, upstream's `eqs=` and `g=` from its "ok:" line, and the fingerprint.  Every case is also checked
against the numpy restatement tests/label_model.py where the library is built.  The cases, and what each is for, are listed in cases()."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import label_model  # noqa: E402
from ldpc_testlib import load_base_matrix  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
EXE = os.path.join(ROOT, "oracle", "_ref", "label_ref")

DRIVER = r"""
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include "commons_portable.h"
#include "code_generation.h"

// ---- the symbols of commons_portable.cpp on the path of generate_code
int initial_random_seed = 1;
std::mt19937 generator(-1);
static bool random_initialized = false;
void reset_random() { random_initialized = false; }
void ensure_random_is_initialized() {
    if (!random_initialized) { generator = std::mt19937(initial_random_seed); random_initialized = true; }
}
int next_random_int(int lo, int hi) {
    ensure_random_is_initialized();
    std::uniform_int_distribution<int> dist(lo, hi - 1);
    return dist(generator);
}
double next_random_01() {   // combinatorics.cpp links against it; generate_code never calls it
    ensure_random_is_initialized();
    std::uniform_real_distribution<double> dist;
    return dist(generator);
}
[[noreturn]] void die(char const *format, ...) {
    va_list ap; va_start(ap, format); vfprintf(stderr, format, ap); va_end(ap);
    fputs("\n", stderr);
    exit(1);
}
std::string format_to_string(char const *, ...) { return std::string(); }
exception_wrapper::~exception_wrapper() {}
void console_digest_exception_wrapper(char, std::string const &, exception_wrapper *w) { delete w; }
console_message_hook::console_message_hook(char s, std::string const &, std::string const &) : symbol(s) {}
console_message_hook::~console_message_hook() {}
console_exception_hook::~console_exception_hook() {}
void console_check_hooks() {}

int main() {
    int rh, nh, g, M, A, seed, K;
    if (scanf("%d %d %d %d %d %d %d", &rh, &nh, &g, &M, &A, &seed, &K) != 7) return 2;
    matrix<int> proto(rh, nh), result;
    for (int i = 0; i < rh; ++i)
        for (int j = 0; j < nh; ++j)
            if (scanf("%d", &proto(i, j)) != 1) return 2;
    initial_random_seed = seed;
    reset_random();
    for (int k = 0; k < K; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = generate_code(proto, g, M, A, result);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("\n@@call %d %.6f", ok ? 1 : 0, sec);
        if (ok)
            for (int i = 0; i < rh; ++i)
                for (int j = 0; j < nh; ++j) printf(" %d", result(i, j));
        printf("\n");
    }
    printf("@@fingerprint");
    for (int i = 0; i < 8; ++i) printf(" %d", next_random_int(0, 1 << 30));
    printf("\n");
    return 0;
}
"""

SMALL = np.array([[1, 1, 0, 1, 1, 0], [1, 0, 1, 1, 0, 1], [0, 1, 1, 0, 1, 1]])   # 3 x 6
K23 = np.ones((2, 3), dtype=np.int64)
SAME_COLUMNS = np.array([[1, 1, 1, 0], [0, 0, 1, 1]])
FIXED_PAIR = np.array([[2, 2, 1, 1], [2, 2, 1, 1]])   # every labelling has equal columns 0 and 1


def appendix_c():
    """The Appendix C protograph with the shipped search's conventions: 1 where a shift is present, 2 where the shift is 0 inside the
    first 16 columns (the dual diagonal)."""
    H = load_base_matrix()
    fixed = (H == 0) & (np.arange(H.shape[1])[None, :] < H.shape[0])
    proto = np.where(H < 0, 0, np.where(fixed, 2, 1))
    assert int((proto > 0).sum()) == 112 and int((proto == 2).sum()) == 32   # diagonal 16, subdiagonal 15, top of column 15
    return proto


def cases():
    """name -> (proto [rh, nh], target_girth, M, max_attempts, seed, K calls)"""
    out = {}
    for g in (6, 8, 10):          # 3, 11 and 20 equations; M = 7, g = 10 exhausts
        for M in (7, 31):
            out["small_g%d_m%d" % (g, M)] = (SMALL, g, M, 100000, 1, 3)
    for g in (12, 14, 16):        # the tree allows girth 12: beyond it no draw is made
        out["k23_g%d_m50" % g] = (K23, g, 50, 1000, 1, 1)
    out["same_columns_m3"] = (SAME_COLUMNS, 6, 3, 1000, 1, 6)   # no equations; the sixth call meets equal columns
    # M = 32513: 2^32 mod M = 32509, the largest rejection rate below 2^15.  Every attempt has equal columns: all draws are consumed
    out["redraw_seed357"] = (FIXED_PAIR, 4, 32513, 1000, 357, 1)     # word 776 is redrawn: the first word of an attempt
    out["redraw_seed105"] = (FIXED_PAIR, 4, 32513, 2000, 105, 1)     # words 4165 (inside) and 6644 (last word of an attempt)
    out["small_redraw_seed531"] = (SMALL, 8, 32513, 100000, 531, 4)   # word 6, inside the first attempt, in front of every accept
    out["small_redraw_seed1298"] = (SMALL, 8, 32513, 100000, 1298, 6)  # word 33, in the third attempt
    appc = appendix_c()
    out["appc_g6_m126"] = (appc, 6, 126, 1000000, 1, 4)
    out["appc_g6_m126_two_calls"] = (appc, 6, 126, 1000000, 1, 2)   # the sequence of tests/cpp/label_driver.cpp
    out["appc_g8_m399"] = (appc, 8, 399, 1000000, 1, 1)              # the retry of main_good_code_search.cpp:298
    out["appc_g8_m126_a2000"] = (appc, 8, 126, 2000, 1, 1)           # exhausts
    return out


def build_reference(opt="-O2", exe=EXE):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(os.path.dirname(exe), "label_ref_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", opt, "-w", "-I", REF, src] +
                          [os.path.join(REF, n) for n in ("code_generation.cpp", "equations.cpp", "data_structures.cpp", "combinatorics.cpp")] +
                          ["-o", exe])
    return exe


def reference(proto, g, M, A, seed, K, exe=EXE):
    """upstream on one case: the golden's fields and the seconds each call took"""
    proto = np.asarray(proto)
    words = [proto.shape[0], proto.shape[1], g, M, A, seed, K] + [int(v) for v in proto.reshape(-1)]
    text = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True, check=True).stdout
    parts = text.split("@@call ")
    calls, seconds, eqs, tree_girth = [], [], None, None
    for before, own in zip(parts[:-1], parts[1:]):
        fields = own.split("\n")[0].split()
        ok = fields[0] == "1"
        seconds.append(float(fields[1]))
        m = re.search(r"ok: g=(\d+), eqs=(\d+)", before)
        if m:
            tree_girth, eqs = int(m.group(1)), int(m.group(2))
        t = re.search(r"codes selected, (\d+) tested", before)
        assert ok == (t is not None)
        calls.append({"ok": ok, "attempts": int(t.group(1)) if ok else (A if m else 0),
                      "matrix": np.array(fields[2:], dtype=np.int64).reshape(proto.shape).tolist() if ok else None})
    fp = [int(v) for v in text.split("@@fingerprint")[1].split()]
    assert len(calls) == K and len(fp) == 8
    return {"proto": proto.tolist(), "target_girth": g, "M": M, "max_attempts": A, "seed": seed, "calls": calls, "eqs": eqs,
            "tree_girth": tree_girth, "fingerprint": fp}, seconds


def check_model(name, gold):
    import ldpc_lib_amd
    table = ldpc_lib_amd.label_equations(gold["proto"], gold["target_girth"])
    if gold["eqs"] is not None:
        assert (table["n_equations"], table["tree_girth"]) == (gold["eqs"], gold["tree_girth"]), (name, table["n_equations"], table["tree_girth"])
    else:
        assert table["tree_girth"] < gold["target_girth"], name
    stream = label_model.Stream(seed=gold["seed"])
    for k, call in enumerate(gold["calls"]):
        ok, attempts, H = label_model.generate_code(gold["proto"], table, gold["target_girth"], gold["M"], gold["max_attempts"], stream)
        assert (ok, attempts) == (call["ok"], call["attempts"]), (name, k, ok, attempts, call["ok"], call["attempts"])
        assert not ok or H.tolist() == call["matrix"], (name, k)
    assert stream.fingerprint() == gold["fingerprint"], name


def main(argv):
    assert os.path.isdir(REF), f"the upstream tree is not mounted at {REF}"
    build_reference()
    os.makedirs(label_model.LABEL_GOLDEN_DIR, exist_ok=True)
    for name, (proto, g, M, A, seed, K) in cases().items():
        if argv and name not in argv:
            continue
        gold, seconds = reference(proto, g, M, A, seed, K)
        path = os.path.join(label_model.LABEL_GOLDEN_DIR, name + ".json")
        with open(path, "w") as f:
            json.dump(gold, f, separators=(",", ":"))
            f.write("\n")
        try:
            check_model(name, gold)
            model = "model agrees"
        except ImportError:
            model = "model not checked (library not built)"
        print(f"{name}: eqs {gold['eqs']}, tree girth {gold['tree_girth']}, calls {[(c['ok'], c['attempts']) for c in gold['calls']]}, "
              f"{sum(seconds):.3f} s, {os.path.getsize(path)} bytes, {model}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
