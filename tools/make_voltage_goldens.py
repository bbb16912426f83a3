#!/usr/bin/env python3
"""Golden results of the voltage check and of the bank search from the COMPILED UPSTREAM SOURCES: equation_builder::check_voltages and
check_voltages_and_coefs (equations.cpp, with graph_spider.h, data_structures.cpp, combinatorics.cpp).

Run where the upstream tree is mounted (REF, default as in oracle/Makefile):

    python3 tools/make_voltage_goldens.py [case names...]

It compiles those three upstream files unchanged, with the driver below, into oracle/_ref/voltage_ref (never committed).  The driver
supplies the symbols of commons_portable.cpp as tools/make_label_goldens.py does, except that die() THROWS: "upstream exits" (a zero
voltage sum rescued by its coefficients reaches divisors(0)) is recorded as a field of the labelling.  It builds the Tanner graph as
search_ggp/read_and_construct_equations.cpp does and then either checks K labellings read from standard input, or restates the loop of
search_ggp/random_search_bank_good_codes.cpp with a budget -- the unbounded check_voltages(a), upstream's acceptance -- and draws eight
next_random_int(0, 1 << 30) as a fingerprint of the generator.  It writes tests/golden/voltage/check.json and bank.json, a line per case:
upstream's results alone, a failed set as its size and CRC-32; the inputs are the cases below, held under a CRC (see goldens()).  Every case is also
checked against the numpy restatement tests/voltage_model.py where the library is built, and main() asserts that the cases hold what
they are for.  The cases are listed in check_cases() and bank_cases()."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import label_model  # noqa: E402
import voltage_model as vm  # noqa: E402
from ldpc_testlib import load_base_matrix  # noqa: E402
from make_label_goldens import K23, SAME_COLUMNS, SMALL, appendix_c  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
EXE = os.path.join(ROOT, "oracle", "_ref", "voltage_ref")
REDRAW_FOUR = np.array([[2, 2, 1, 1], [2, 0, 1, 1]])   # four draws per attempt, as the redraw streams of the label goldens; three equations at g = 6

DRIVER = r"""
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>
#include "commons_portable.h"
#include "equations.h"

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
double next_random_01() {
    ensure_random_is_initialized();
    std::uniform_real_distribution<double> dist;
    return dist(generator);
}
void die(char const *format, ...) {   // upstream prints and exits; here the caller records it
    char buf[512];
    va_list ap; va_start(ap, format); vsnprintf(buf, sizeof buf, format, ap); va_end(ap);
    throw std::runtime_error(buf);
}
std::string format_to_string(char const *, ...) { return std::string(); }
exception_wrapper::~exception_wrapper() {}
void console_digest_exception_wrapper(char, std::string const &, exception_wrapper *w) { delete w; }
console_message_hook::console_message_hook(char s, std::string const &, std::string const &) : symbol(s) {}
console_message_hook::~console_message_hook() {}
console_exception_hook::~console_exception_hook() {}
void console_check_hooks() {}

static void print_result(voltage_check_result const &r) {
    if (r.first_failed_equation != -1) { printf("@@v %d\n", r.first_failed_equation); return; }
    printf("@@v -1 %d %d %zu", r.min_ok_modulo, r.max_nonok_modulo, r.failed_modulos.size());
    for (int m : r.failed_modulos) printf(" %d", m);
    printf("\n");
}

int main() {
    int bank, rh, nh, g;
    if (scanf("%d %d %d %d", &bank, &rh, &nh, &g) != 4) return 2;
    std::vector<int> am;
    std::vector<int> proto((size_t)rh * nh);
    for (int &v : proto) if (scanf("%d", &v) != 1) return 2;
    graph< vector_bag > tanner;
    int edges = 0;
    for (int c = 0; c < nh; ++c)
        for (int r = 0; r < rh; ++r)
            if (proto[(size_t)r * nh + c] > 0) {
                vector_bag fw(edges++);
                tanner.add_bidi_edge(c, r + nh, fw, -fw);
                am.push_back(proto[(size_t)r * nh + c]);
            }
    equation_builder eq(tanner, g);
    printf("@@eq %d %d\n", eq.n_equations(), eq.tree_girth());
    std::vector<int> a((size_t)edges), coef((size_t)edges);
    if (!bank) {
        int max_modulo, K, has_coef, unbounded;
        if (scanf("%d %d %d %d", &max_modulo, &K, &has_coef, &unbounded) != 4) return 2;
        double sec = 0;
        for (int k = 0; k < K; ++k) {
            for (int &v : a) if (scanf("%d", &v) != 1) return 2;
            if (has_coef) for (int &v : coef) if (scanf("%d", &v) != 1) return 2;
            try {
                const auto t0 = std::chrono::steady_clock::now();
                voltage_check_result r = has_coef ? eq.check_voltages_and_coefs(a, max_modulo, coef, 16) : unbounded ? eq.check_voltages(a) : eq.check_voltages(a, max_modulo);
                sec += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                print_result(r);
            } catch (std::runtime_error const &e) {
                printf("@@die %s\n", e.what());
            }
        }
        printf("@@seconds %.6f\n", sec);
        return 0;
    }
    int T, exact, A, want, seed;
    if (scanf("%d %d %d %d %d", &T, &exact, &A, &want, &seed) != 5) return 2;
    initial_random_seed = seed;
    reset_random();
    int tested = 0, ok_codes = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int round = 0; round < A && ok_codes < want; ++round) {
        for (int i = 0; i < edges; ++i) a[(size_t)i] = am[(size_t)i] == 1 ? next_random_int(0, T) : 0;
        voltage_check_result res = eq.check_voltages(a);
        tested = round + 1;
        if (res.first_failed_equation == -1 && res.min_ok_modulo <= T && (exact == 0 || res.check_modulo(exact))) {
            ++ok_codes;
            printf("@@ok %d %d", round, res.min_ok_modulo);
            for (int v : a) printf(" %d", v);
            printf("\n");
        }
    }
    printf("@@seconds %.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf("@@tested %d\n@@fingerprint", tested);
    for (int i = 0; i < 8; ++i) printf(" %d", next_random_int(0, 1 << 30));
    printf("\n");
    return 0;
}
"""


def shipped_labelling():
    """the Appendix C labelling as voltages: its shifts, column by column with the rows ascending"""
    H = load_base_matrix()
    rows, cols, _ = label_model.layout(H >= 0)
    return H[rows, cols].astype(np.int64)


def labellings(rng, K, E, below, first=()):
    """K labellings below `below`; after those of `first`: the all-zero one and one with a single non-zero edge, where K leaves room"""
    V = rng.randint(0, below, size=(K, E)).astype(np.int64)
    special = [np.asarray(v) for v in first]
    if K >= 63:
        single = np.zeros(E, dtype=np.int64)
        single[int(rng.randint(E))] = 1 + int(rng.randint(below - 1)) if below > 2 else 1
        special += [np.zeros(E, dtype=np.int64), single]
    for i, v in enumerate(special):
        V[i] = v
    return V


def check_cases():
    """name -> (proto, target_girth, max_modulo, voltages [K, E], coefs [K, E] or None).  Together: K in {1, 63, 64, 65, 200}, max_modulo
    in {1, 2, 3, 63, 64, 65, 127, 128, 1000, 65535}, voltages below 2, 7, 31, 126 and 32767, coefficients below 3 and 15."""
    rng = np.random.RandomState(2031)
    out = {}
    E = int((SMALL > 0).sum())
    for g, K, below, mm in ((6, 1, 2, 1), (6, 63, 7, 2), (8, 64, 31, 3), (8, 65, 126, 63), (10, 200, 31, 64), (10, 64, 32767, 65535), (8, 65, 32767, 1000),
                            (6, 63, 126, 65), (10, 65, 7, 127), (8, 1, 31, 128), (6, 64, 2, 3)):
        out["small_g%d_k%d_v%d_m%d" % (g, K, below, mm)] = (SMALL, g, mm, labellings(rng, K, E, below), None)
    for g, K, below, mm, cbelow in ((10, 65, 31, 64, 15), (10, 64, 7, 128, 3), (8, 65, 7, 63, 3), (6, 63, 2, 2, 15)):   # g = 10: status 1 and 2
        out["small_coef_g%d_k%d_v%d_m%d_c%d" % (g, K, below, mm, cbelow)] = (SMALL, g, mm, labellings(rng, K, E, below), rng.randint(0, cbelow, size=(K, E)))
    out["k23_g14_m127"] = (K23, 14, 127, labellings(rng, 64, 6, 31), None)                 # the tree allows 12
    out["same_columns_m64"] = (SAME_COLUMNS, 6, 64, labellings(rng, 65, 5, 7), None)       # no equations: the empty set
    appc = (appendix_c() > 0).astype(np.int64)
    ship = shipped_labelling()
    out["appc_g6_m1000"] = (appc, 6, 1000, labellings(rng, 64, 112, 126, [ship]), None)    # 343 equations
    big = labellings(rng, 65, 112, 126, [ship])
    big[40:] = rng.randint(0, 32767, size=(25, 112))                                       # no zero sum; every modulo up to 127 fails
    out["appc_g8_m127"] = (appc, 8, 127, big, None)                                        # 5200 equations: three tiles
    return out


def bank_cases():
    """name -> (proto, target_girth, T, exact_modulo, max_attempts, want, seed)"""
    appc = appendix_c()
    return {
        "bank_small_g8_t31": (SMALL, 8, 31, 0, 2000, 200, 1),
        "bank_small_g8_t31_exact62": (SMALL, 8, 31, 62, 2000, 200, 1),   # 62 divides some accepted attempt's sum
        "bank_small_g8_t31_exhausts": (SMALL, 8, 31, 0, 300, 1000, 3),
        "bank_appc_g6_t126": (appc, 6, 126, 0, 3000, 3000, 1),            # the shipped conventions: 32 fixed edges; exhausts
        "bank_appc_g6_t126_exact252": (appc, 6, 126, 252, 3000, 25, 1),
        "bank_k23_g14_t50": (K23, 14, 50, 0, 500, 5, 1),                  # no early return: the equations shorter than 12
        "bank_redraw_seed531": (SMALL, 8, 32513, 0, 100, 5, 531),         # word 6 is redrawn, inside the first attempt
        "bank_redraw_seed357": (REDRAW_FOUR, 6, 32513, 0, 1000, 300, 357),  # word 776 is redrawn: the first word of attempt 194
    }


def build_reference(opt="-O2", exe=EXE):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(os.path.dirname(exe), "voltage_ref_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", opt, "-w", "-I", REF, src] +
                          [os.path.join(REF, n) for n in ("equations.cpp", "data_structures.cpp", "combinatorics.cpp")] + ["-o", exe])
    return exe


def run(words, exe=EXE):
    return subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True, check=True).stdout


def header(text):
    eqs, tree_girth = (int(v) for v in text.split("@@eq ")[1].split("\n")[0].split())
    return eqs, tree_girth, float(text.split("@@seconds ")[1].split()[0])


def reference_check(proto, g, max_modulo, V, Cf, unbounded=False, exe=EXE):
    """upstream on K labellings: the golden's fields and the seconds the K calls took"""
    proto, V = np.asarray(proto), np.asarray(V)
    words = [0, proto.shape[0], proto.shape[1], g, *proto.reshape(-1), max_modulo, len(V), int(Cf is not None), int(unbounded)]
    for k in range(len(V)):
        words += list(V[k]) + (list(Cf[k]) if Cf is not None else [])
    text = run(words, exe)
    eqs, tree_girth, seconds = header(text)
    results, died = [], set()
    for line in text.split("\n"):
        f = line.split()
        if line.startswith("@@die"):
            results.append(2)
            died.add(line[6:])
        elif line.startswith("@@v") and f[1] != "-1":
            assert f[1] == "0"
            results.append(1)
        elif line.startswith("@@v"):
            assert len(f) == 5 + int(f[4])
            results.append([int(f[2]), int(f[3]), *digest([int(v) for v in f[5:]])])
    assert len(results) == len(V) and len(died) <= 1
    return {"kind": "check", "inputs_crc": crc(proto, V, Cf), "eqs": eqs, "tree_girth": tree_girth, "died": died.pop() if died else None,
            "results": results}, seconds


def reference_bank(proto, g, T, exact, A, want, seed, exe=EXE):
    proto = np.asarray(proto)
    text = run([1, proto.shape[0], proto.shape[1], g, *proto.reshape(-1), T, exact, A, want, seed], exe)
    eqs, tree_girth, seconds = header(text)
    accepted = [[int(v) for v in line.split()[1:]] for line in text.split("\n") if line.startswith("@@ok")]
    return {"kind": "bank", "inputs_crc": crc(proto, [g, T, exact, A, want, seed]), "eqs": eqs, "tree_girth": tree_girth, "accepted": [a[0] for a in accepted],
            "min_ok": [a[1] for a in accepted], "labellings_crc": crc([a[2:] for a in accepted]), "attempts_tested": int(text.split("@@tested ")[1].split()[0]),
            "fingerprint": [int(v) for v in text.split("@@fingerprint")[1].split()]}, seconds


def crc(*arrays):
    """CRC-32 over the int32 values of the arrays, None left out"""
    c = 0
    for a in arrays:
        if a is not None:
            c = zlib.crc32(np.ascontiguousarray(a, dtype="<i4").tobytes(), c)
    return c


def digest(failed):
    """a failed set as the goldens keep it: [number of members, CRC-32 of the ascending members]"""
    return [len(failed), crc(failed)]


def status_of(result):
    return 2 if "died" in result else 0 if result["first_failed"] == -1 else 1


def goldens(only=None):
    """name -> a case of check_cases() / bank_cases() with what the compiled upstream sources gave for it (tests/golden/voltage/).  The
    files hold upstream's results alone, a failed set as digest(); the inputs are the cases', under a CRC.  Check cases: proto,
    target_girth, max_modulo, voltages, coefs, eqs, tree_girth, results = per labelling {"died": message}, {"first_failed": 0} or
    {"first_failed": -1, "min_ok", "max_nonok", "failed": digest}.  Bank cases: the case's parameters, eqs, tree_girth, accepted
    (attempt indices), min_ok, labellings_crc (over the accepted labellings' voltages, attempt by attempt), attempts_tested, fingerprint."""
    out = {}
    for name, (proto, g, mm, V, Cf) in check_cases().items():
        if only and name != only:
            continue
        gold = vm.load_golden("check")[name]
        assert gold["inputs_crc"] == crc(proto, V, Cf), name
        results = [{"died": gold["died"]} if r == 2 else {"first_failed": 0} if r == 1 else
                   {"first_failed": -1, "min_ok": r[0], "max_nonok": r[1], "failed": r[2:]} for r in gold["results"]]
        out[name] = {"kind": "check", "proto": np.asarray(proto, dtype=np.int16), "target_girth": g, "max_modulo": mm, "voltages": np.asarray(V).tolist(),
                     "coefs": None if Cf is None else np.asarray(Cf).tolist(), "eqs": gold["eqs"], "tree_girth": gold["tree_girth"], "results": results}
    for name, (proto, g, T, exact, A, want, seed) in bank_cases().items():
        if only and name != only:
            continue
        gold = vm.load_golden("bank")[name]
        assert gold["inputs_crc"] == crc(proto, [g, T, exact, A, want, seed]), name
        out[name] = dict(gold, proto=np.asarray(proto, dtype=np.int16), target_girth=g, T=T, exact_modulo=exact, max_attempts=A, want=want, seed=seed)
    return out


def check_model(name, gold):
    """the numpy restatement against one golden, every field upstream defines; returns the model's results of a check case"""
    import ldpc_lib_amd
    if gold["kind"] == "check":
        table = ldpc_lib_amd.label_equations(vm.all_random(gold["proto"]), gold["target_girth"])
        assert (table["n_equations"], table["tree_girth"]) == (gold["eqs"], gold["tree_girth"]), (name, table["n_equations"], table["tree_girth"])
        model = vm.check_voltages(table, gold["voltages"], gold["max_modulo"], gold["coefs"])
        for k, (m, r) in enumerate(zip(model, gold["results"])):
            assert m["status"] == status_of(r), (name, k, m["status"], r)
            if m["status"] == 0:
                assert (m["min_ok"], m["max_nonok"], digest(m["failed"])) == (r["min_ok"], r["max_nonok"], r["failed"]), (name, k)
            if m["status"] == 2:
                assert r["died"] == "global_divisor_table is called with the argument 0", (name, k, r)
        return model
    table = ldpc_lib_amd.label_equations(gold["proto"], gold["target_girth"])
    assert table["tree_girth"] == gold["tree_girth"], name
    stream = label_model.Stream(seed=gold["seed"])
    got, tested = vm.bank(gold["proto"], table, gold["T"], gold["exact_modulo"], gold["max_attempts"], gold["want"], stream)
    rows, cols, _ = label_model.layout(gold["proto"])
    assert ([i for i, _, _ in got], [m for _, m, _ in got]) == (gold["accepted"], gold["min_ok"]), name
    assert crc([H[rows, cols] for _, _, H in got]) == gold["labellings_crc"], name
    assert tested == gold["attempts_tested"] and stream.fingerprint() == gold["fingerprint"], name
    return None


def main(argv):
    assert os.path.isdir(REF), f"the upstream tree is not mounted at {REF}"
    build_reference()
    os.makedirs(vm.VOLTAGE_GOLDEN_DIR, exist_ok=True)
    seen = {"status": set(), "all_fail": 0, "empty": 0}
    jobs = [(n, c, reference_check) for n, c in check_cases().items()] + [(n, c, reference_bank) for n, c in bank_cases().items()]
    for name, case, ref in jobs:
        if argv and name not in argv:
            continue
        gold, seconds = ref(*case)
        path = vm.golden_path(gold["kind"])
        held = vm.load_golden(gold["kind"]) if os.path.exists(path) else {}
        held[name] = gold
        with open(path, "w") as f:   # one case per line
            f.write("{\n" + ",\n".join(json.dumps(n) + ":" + json.dumps(held[n], separators=(",", ":")) for n in sorted(held)) + "\n}\n")
        gold = goldens(name)[name]
        if gold["kind"] == "check":
            for r in gold["results"]:
                seen["status"].add(status_of(r))
                if status_of(r) == 0:
                    seen["all_fail"] += gold["max_modulo"] >= 2 and r["min_ok"] == gold["max_modulo"] + 1
                    seen["empty"] += r["failed"][0] == 0
            what = "statuses %s" % np.bincount([status_of(r) for r in gold["results"]], minlength=3).tolist()
        else:
            assert len(gold["accepted"]) >= 2, name
            what = "%d accepted, %d tested" % (len(gold["accepted"]), gold["attempts_tested"])
        try:
            check_model(name, gold)
            model = "model agrees"
        except ImportError:
            model = "model not checked (library not built)"
        print(f"{name}: eqs {gold['eqs']}, tree girth {gold['tree_girth']}, {what}, {seconds:.3f} s, {model}", flush=True)
    if not argv:
        assert seen["status"] == {0, 1, 2} and seen["all_fail"] >= 1 and seen["empty"] >= 1, seen


if __name__ == "__main__":
    main(sys.argv[1:])
