"""The voltage check and the bank search on the GPU (ldpc_hip_check_voltages, ldpc_hip_label_bank; csrc/ldpc_voltage.hpp): every field of
every golden of the compiled upstream sources (tests/golden/voltage/), the status 2 fields and max |sum| against the numpy restatement
(tests/voltage_model.py), the same under forced pieces, forced rounds and the alternative kernel layout, a generator that does not
stand at a block boundary, random protographs against the model, the bank's labellings fed back through the check, the accepted
labellings under the girth trace (an independent implementation), and the C++ layer (include/ldpc/equations.h).  Everything is integer:
equality throughout."""
import os
import subprocess
import sys

import numpy as np
import pytest

import label_model as lm
import voltage_model as vm
from ldpc_testlib import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_voltage_goldens as mvg  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDENS = mvg.goldens()   # the tool's cases joined with upstream's results: a failed set is there as [size, CRC-32]
CHECKS = sorted(n for n, g in GOLDENS.items() if g["kind"] == "check")
BANKS = sorted(n for n, g in GOLDENS.items() if g["kind"] == "bank")
_MODEL = {}


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def model_of(L, name):
    """the model's results of a check golden, computed once"""
    if name not in _MODEL:
        g = GOLDENS[name]
        table = L.label_equations(vm.all_random(g["proto"]), g["target_girth"])
        _MODEL[name] = vm.check_voltages(table, g["voltages"], g["max_modulo"], g["coefs"])
    return _MODEL[name]


def assert_equals_golden(L, name):
    """every field upstream defines against the golden; where upstream exits (status 2) and max |sum| against the model"""
    g = GOLDENS[name]
    out = L.check_voltages(g["proto"], g["target_girth"], g["voltages"], g["max_modulo"], g["coefs"])
    assert (out["n_equations"], out["tree_girth"]) == (g["eqs"], g["tree_girth"])
    assert out["failed"].shape == (len(g["voltages"]), g["max_modulo"] // 64 + 1)
    for k, (r, m) in enumerate(zip(g["results"], model_of(L, name))):
        failed = L.failed_moduli(out["failed"][k]).tolist()
        got = (int(out["status"][k]), int(out["min_ok"][k]), int(out["max_nonok"][k]), failed)
        if "died" in r:
            assert got == (2, m["min_ok"], m["max_nonok"], m["failed"]), (name, k)
        elif r["first_failed"] == -1:
            assert got[:3] == (0, r["min_ok"], r["max_nonok"]) and mvg.digest(failed) == r["failed"], (name, k, failed, m["failed"])
        else:
            assert got == (1, 0, 0, []), (name, k)
        assert int(out["max_abs_sum"][k]) == m["max_abs_sum"], (name, k)
    return out


@pytest.mark.parametrize("name", CHECKS)
def test_check_voltages_equals_golden(L, torch, name):
    assert_equals_golden(L, name)


@pytest.mark.parametrize("name", ["small_g6_k1_v2_m1", "small_g10_k64_v32767_m65535", "small_coef_g10_k65_v31_m64_c15", "same_columns_m64", "appc_g6_m1000",
                                  "appc_g8_m127"])
def test_the_moduli_layout_gives_the_same(L, torch, monkeypatch, name):
    """the layout kept for measurements: the smallest and the largest max_modulo, coefficients, no equations, one tile and three"""
    monkeypatch.setenv("LDPC_HIP_VOLTAGE_LAYOUT", "moduli")
    assert_equals_golden(L, name)


@pytest.mark.parametrize("piece", [1, 65])
@pytest.mark.parametrize("name", ["small_g10_k200_v31_m64", "small_coef_g10_k65_v31_m64_c15", "small_g8_k65_v32767_m1000", "appc_g8_m127", "appc_g6_m1000"])
def test_forced_pieces_change_nothing(L, torch, monkeypatch, name, piece):
    """200 labellings in pieces of 65 end on a piece of 5; 65 in pieces of 65 are one piece, in pieces of 1 sixty-five; 64 one short piece."""
    monkeypatch.setenv("LDPC_HIP_VOLTAGE_PIECE", str(piece))
    assert_equals_golden(L, name)


def test_one_labelling_and_no_bitmap(L, torch):
    """[E] in place of [K, E], and the C entry point with failed = NULL and without tree_girth / n_equations"""
    g = GOLDENS["appc_g6_m1000"]
    out = L.check_voltages(g["proto"], 6, g["voltages"][0], 1000)
    assert (out["status"].tolist(), out["min_ok"].tolist(), out["max_nonok"].tolist()) == ([0], [79], [215])
    assert len(L.failed_moduli(out["failed"][0])) == 140
    lib = L.load_library()
    P = np.ascontiguousarray(g["proto"], dtype=np.int16)
    V = np.ascontiguousarray(g["voltages"], dtype=np.int32)
    res = [np.zeros(len(V), dtype=np.int32) for _ in range(4)]
    assert lib.ldpc_hip_check_voltages(16, 32, P.ctypes.data, 6, 1000, V.ctypes.data, None, len(V), 0, *[r.ctypes.data for r in res], None, None, None) == 0
    full = L.check_voltages(g["proto"], 6, V, 1000)
    assert all(np.array_equal(r, full[key]) for r, key in zip(res, ("status", "min_ok", "max_nonok", "max_abs_sum")))


def random_cases():
    rng = np.random.RandomState(2031)
    out = []
    while len(out) < 24:
        rh, nh = int(rng.randint(3, 7)), int(rng.randint(6, 13))
        proto = (rng.rand(rh, nh) < 0.5).astype(np.int16)
        proto[rng.rand(rh, nh) < 0.08] = 2 + int(rng.randint(0, 3))   # any positive value is an edge
        E = int((proto > 0).sum())
        if E < 4:
            continue
        below = int(rng.choice([2, 7, 31, 126, 32767]))
        out.append((proto, int(rng.choice([6, 8])), int(rng.choice([1, 2, 63, 64, 127, 1000, 65535])), rng.randint(0, below, size=(20, E)),
                    rng.randint(0, int(rng.choice([3, 15])), size=(20, E)) if rng.rand() < 0.5 else None))
    return out


@pytest.mark.parametrize("case", range(24))
def test_random_protographs_equal_the_model(L, torch, case):
    proto, g, mm, V, Cf = random_cases()[case]
    table = L.label_equations(vm.all_random(proto), g)
    model = vm.check_voltages(table, V, mm, Cf)
    out = L.check_voltages(proto, g, V, mm, Cf)
    print(case, proto.shape, g, mm, table["n_equations"], np.bincount([m["status"] for m in model], minlength=3))
    assert (out["n_equations"], out["tree_girth"]) == (table["n_equations"], table["tree_girth"])
    for k, m in enumerate(model):
        got = {"status": int(out["status"][k]), "max_abs_sum": int(out["max_abs_sum"][k]), "min_ok": int(out["min_ok"][k]),
               "max_nonok": int(out["max_nonok"][k]), "failed": L.failed_moduli(out["failed"][k]).tolist()}
        assert got == m, (case, k)


# ---- the bank search

def words_after(state, pos, n=8):
    return lm.Stream(state=state, pos=pos).fingerprint()[:n]


def run_bank_golden(L, g):
    state, pos = lm.Stream(seed=g["seed"]).state()
    codes, min_ok, index, tested, tree_girth, (s1, p1) = L.label_bank(g["proto"], g["target_girth"], g["T"], g["max_attempts"], state, pos, want=g["want"],
                                                                      exact_modulo=g["exact_modulo"])
    rows, cols, _ = lm.layout(g["proto"])
    assert tree_girth == g["tree_girth"]
    assert (index.tolist(), min_ok.tolist()) == (g["accepted"], g["min_ok"])
    assert mvg.crc(codes[:, rows, cols]) == g["labellings_crc"]
    assert all((c[g["proto"] == 0] == -1).all() for c in codes)
    assert tested == g["attempts_tested"]
    assert words_after(s1, p1) == g["fingerprint"]
    return codes, min_ok


@pytest.mark.parametrize("name", BANKS)
def test_label_bank_equals_golden(L, torch, name):
    run_bank_golden(L, GOLDENS[name])


@pytest.mark.parametrize("n", [1, 3, 64, 1000])
@pytest.mark.parametrize("name", BANKS)
def test_forced_rounds_change_nothing(L, torch, monkeypatch, name, n):
    """Round boundaries inside the run; with rounds of 1 and 3 attempts the redraws of the T = 32513 cases are the first or an inner
    word of a round (776 = 4 * 194 opens attempt 194 of seed 357; word 6 is inside attempt 0 of seed 531)."""
    g = GOLDENS[name]
    monkeypatch.setenv("LDPC_HIP_LABEL_ROUND", str(n))
    run_bank_golden(L, g)
    if g["attempts_tested"] > n:
        assert L.label_last_stats()[0] > 1, "more than one round"


def test_redraws_are_met_where_the_goldens_place_them(L, torch):
    for name, count in (("bank_redraw_seed531", 1), ("bank_redraw_seed357", 1)):
        run_bank_golden(L, GOLDENS[name])
        assert L.label_last_stats()[1] == count, name
    assert lm.redraw_positions(lm.Stream(seed=357).peek(1200), 32513).tolist() == [776]
    assert lm.redraw_positions(lm.Stream(seed=531).peek(60), 32513).tolist() == [6]


@pytest.mark.parametrize("burn", [1000, 623, 624, 1])
def test_generator_inside_a_block(L, torch, burn):
    """pos_in anywhere in the 624-word block, the end of the block included"""
    g = GOLDENS["bank_small_g8_t31_exact62"]
    table = L.label_equations(g["proto"], 8)
    stream = lm.Stream(seed=77).advance(burn)
    state, pos = stream.state()
    assert pos == (burn if burn <= 624 else burn - 624)
    codes, min_ok, index, tested, _, (s1, p1) = L.label_bank(g["proto"], 8, 31, 500, state, pos, want=30, exact_modulo=62)
    got, at = vm.bank(g["proto"], table, 31, 62, 500, 30, stream)
    assert len(got) == 30 and tested == at
    assert [(int(i), int(m), c.tolist()) for i, m, c in zip(index, min_ok, codes)] == [(i, m, H.tolist()) for i, m, H in got]
    assert words_after(s1, p1) == stream.fingerprint()


@pytest.mark.parametrize("name", BANKS)
def test_the_banks_labellings_pass_the_check_with_the_min_ok_reported(L, torch, name):
    g = GOLDENS[name]
    codes, min_ok = run_bank_golden(L, g)
    rows, cols, _ = lm.layout(g["proto"])
    bound = max(g["T"], g["exact_modulo"])
    out = L.check_voltages(g["proto"], g["target_girth"], codes[:, rows, cols], bound)
    assert (out["status"] == 0).all() and np.array_equal(out["min_ok"], min_ok) and (min_ok <= g["T"]).all()
    if g["exact_modulo"]:
        assert all(g["exact_modulo"] not in L.failed_moduli(row) for row in out["failed"])


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_accepted_labellings_have_the_girth_at_their_smallest_lifting(L, torch, name):
    """The cross-check between two independent implementations, and the only one that does not pass through the equation table:
    EVERY labelling of status 0 with min_ok <= max_modulo of every check golden, and every labelling a bank golden accepts, lifted
    by M = its min_ok, has no cycle below the girth the check was made for -- the target, or what the tree allows -- under the
    girth trace (ldpc_hip_girth_codes).  One trace call per distinct min_ok of the golden."""
    g = GOLDENS[name]
    rows, cols, _ = lm.layout(g["proto"])
    if g["kind"] == "bank":
        codes, min_ok = run_bank_golden(L, g)
        labellings = list(zip(min_ok.tolist(), codes[:, rows, cols].tolist()))
        expected = len(g["accepted"])
    else:
        labellings = [(r["min_ok"], v) for r, v in zip(g["results"], g["voltages"]) if r.get("first_failed") == -1 and r["min_ok"] <= g["max_modulo"]]
        out = L.check_voltages(g["proto"], g["target_girth"], g["voltages"], g["max_modulo"])   # binary: what the lifted graph is about
        expected = int(((out["status"] == 0) & (out["min_ok"] <= g["max_modulo"])).sum())   # with coefficients too: status 0 = no zero sum
    by_m = {}
    for m, v in labellings:
        by_m.setdefault(m, []).append(v)
    done = 0
    for m, vs in sorted(by_m.items()):
        hd = np.full((len(vs), *g["proto"].shape), -1, dtype=np.int16)
        hd[:, rows, cols] = np.array(vs) % m
        S, SA, _ = L.girth_codes(hd, m)
        for s, sa in zip(S, SA):
            girth = L.trace_matrix(s, sa)[0]
            assert girth >= min(g["target_girth"], g["tree_girth"]), (name, m, girth)
            done += 1
    print(name, "labellings traced:", done, "distinct liftings:", len(by_m), "largest:", max(by_m, default=None))
    assert done == len(labellings) == expected


def test_cpp_layer(L, torch, tmp_path):
    """ldpc::check_voltages on a batch and on one labelling, ldpc::check_voltages_and_coefs labelling by labelling -- it throws
    upstream's message where upstream exits -- against the goldens, check_modulo included."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "voltage_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "voltage_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    for name in ("appc_g6_m1000", "small_g10_k200_v31_m64", "small_coef_g10_k64_v7_m128_c3"):
        g = GOLDENS[name]
        mm = g["max_modulo"]
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([*g["proto"].shape, g["target_girth"], mm, len(g["voltages"]), int(g["coefs"] is not None)], dtype=np.int32).tobytes())
            f.write(g["proto"].astype(np.int32).tobytes())
            for k, v in enumerate(g["voltages"]):
                f.write(np.array(v, dtype=np.int32).tobytes())
                if g["coefs"] is not None:
                    f.write(np.array(g["coefs"][k], dtype=np.int32).tobytes())
        out = subprocess.check_output([exe, str(tmp_path / "in.bin")], timeout=120).decode().strip().split("\n")

        def expected(r, m, tag="v"):
            """the driver's line: upstream's fields; the members of the failed set from the model, under upstream's digest"""
            if "died" in r:
                return "die " + r["died"]
            if r["first_failed"] != -1:
                return "%s 0 0 0 0" % tag
            assert mvg.digest(m["failed"]) == r["failed"]
            ok = mm >= r["min_ok"] and (mm > r["max_nonok"] or mm not in m["failed"])
            return " ".join(str(v) for v in [tag, -1, r["min_ok"], r["max_nonok"], int(ok), *m["failed"]])
        model = model_of(L, name)
        assert out[:len(g["results"])] == [expected(r, m) for r, m in zip(g["results"], model)], name
        if g["coefs"] is None:
            assert out[len(g["results"])] == expected(g["results"][0], model[0], "single"), name
        else:
            assert out[len(g["results"])] == "batch 1", name
