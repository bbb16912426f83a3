"""Labelling a protograph under a girth bound on the GPU (ldpc_hip_label_codes, csrc/ldpc_label.hpp): every golden case of the compiled
upstream sources (tests/golden/label/) call by call, the same under forced round sizes, several labellings in one call against chained
calls, a generator that does not stand at a block boundary, random protographs against the numpy restatement (tests/label_model.py),
the accepted Appendix C labellings under the girth trace (an independent implementation), and the C++ layer
(include/ldpc/code_generation.h).  Everything is integer: equality throughout.

Round sizes of 1 and 3 attempts cost one synchronisation per round; they run on the goldens whose calls test at most 5000 attempts in
all (the redraw cases among them), 64 and 1000 on every golden."""
import os
import subprocess

import numpy as np
import pytest

import label_model as lm
from ldpc_testlib import ROOT

pytestmark = pytest.mark.gpu

GOLDENS = lm.load_goldens()
SMALL_ROUNDS_LIMIT = 5000


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def words_after(state, pos, n=8):
    return lm.Stream(state=state, pos=pos).fingerprint()[:n]


def run_golden_calls(L, g):
    """upstream's K calls as K device calls chained through the returned generator; asserts every field of the golden"""
    state, pos = lm.Stream(seed=g["seed"]).state()
    redraws = 0
    for k, call in enumerate(g["calls"]):
        codes, index, tested, tree_girth, (state, pos) = L.label_codes(g["proto"], g["target_girth"], g["M"], g["max_attempts"], state, pos)
        redraws += L.label_last_stats()[1]
        assert len(codes) == (1 if call["ok"] else 0), k
        assert tested == call["attempts"], (k, tested, call["attempts"])
        if g["eqs"] is None:
            assert tree_girth < g["target_girth"]
        else:
            assert tree_girth == g["tree_girth"]
        if call["ok"]:
            assert index.tolist() == [call["attempts"] - 1], k
            assert codes[0].tolist() == call["matrix"], k
    assert words_after(state, pos) == g["fingerprint"]
    return redraws


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_label_codes_equals_golden(L, torch, name):
    run_golden_calls(L, GOLDENS[name])


def total_attempts(g):
    return sum(c["attempts"] for c in g["calls"])


FORCED = [(name, n) for name in sorted(GOLDENS) for n in (1, 3, 64, 1000) if n >= 64 or total_attempts(GOLDENS[name]) <= SMALL_ROUNDS_LIMIT]


@pytest.mark.parametrize("name,n", FORCED)
def test_forced_rounds_change_nothing(L, torch, monkeypatch, name, n):
    """Round boundaries inside the run: with rounds of 1 and 3 attempts every redraw of the M = 32513 cases is the first, an inner or the
    last word of a round (776 = 4 * 194 opens attempt 194; 4165 is inside attempt 1041; 6644 closes attempt 1660)."""
    g = GOLDENS[name]
    monkeypatch.setenv("LDPC_HIP_LABEL_ROUND", str(n))
    run_golden_calls(L, g)
    if g["eqs"] is not None and g["calls"][-1]["attempts"] > n:
        assert L.label_last_stats()[0] > 1, "more than one round"


def test_redraws_are_met_where_the_goldens_place_them(L, torch):
    """The redraw cases consume the words upstream's stream marks: one in seed 357, two in seed 105, one in front of the accepts of
    the 3 x 6 cases; the fingerprint of seed 357 is word 4001 >> 2, not word 4000."""
    assert run_golden_calls(L, GOLDENS["redraw_seed357"]) == 1
    assert run_golden_calls(L, GOLDENS["redraw_seed105"]) == 2
    assert run_golden_calls(L, GOLDENS["small_redraw_seed531"]) == 1
    assert run_golden_calls(L, GOLDENS["small_redraw_seed1298"]) == 1
    s = lm.Stream(seed=357)
    assert lm.redraw_positions(s.peek(4001), 32513).tolist() == [776]
    assert GOLDENS["redraw_seed357"]["fingerprint"][0] == int(s.peek(4002)[4001]) >> 2 == 21485204
    assert lm.redraw_positions(lm.Stream(seed=105).peek(8002), 32513).tolist() == [4165, 6644]


@pytest.mark.parametrize("name", ["appc_g6_m126", "small_g8_m7", "same_columns_m3", "small_redraw_seed1298", "small_g10_m31"])
def test_several_labellings_in_one_call_equal_chained_calls(L, torch, name):
    g = GOLDENS[name]
    K = len(g["calls"])
    assert all(c["ok"] for c in g["calls"])
    state, pos = lm.Stream(seed=g["seed"]).state()
    codes, index, tested, _, (s1, p1) = L.label_codes(g["proto"], g["target_girth"], g["M"], g["max_attempts"], state, pos, want=K)
    ends = np.cumsum([c["attempts"] for c in g["calls"]])
    assert index.tolist() == (ends - 1).tolist() and tested == ends[-1]
    assert codes.tolist() == [c["matrix"] for c in g["calls"]]
    assert words_after(s1, p1) == g["fingerprint"]
    # more than the budget allows: what was found, and all attempts consumed
    few = int(ends[1])
    codes2, index2, tested2, _, (s2, p2) = L.label_codes(g["proto"], g["target_girth"], g["M"], few, state, pos, want=K + 50)
    stream = lm.Stream(seed=g["seed"])
    table = L.label_equations(g["proto"], g["target_girth"])
    got = []
    left = few
    while left > 0:
        ok, n, H = lm.generate_code(g["proto"], table, g["target_girth"], g["M"], left, stream)
        left -= n
        if ok:
            got.append(H.tolist())
    assert codes2.tolist() == got and tested2 == few and len(index2) == len(got) >= 2
    assert words_after(s2, p2) == stream.fingerprint()


@pytest.mark.parametrize("burn", [1000, 623, 624, 1])
def test_generator_inside_a_block(L, torch, burn):
    """pos_in anywhere in the 624-word block, the end of the block included"""
    g = GOLDENS["small_g8_m7"]
    table = L.label_equations(g["proto"], 8)
    stream = lm.Stream(seed=77).advance(burn)
    state, pos = stream.state()
    assert pos == (burn if burn <= 624 else burn - 624)
    codes, index, tested, _, (s1, p1) = L.label_codes(g["proto"], 8, 7, 100000, state, pos, want=5)
    at = 0
    for k in range(5):
        ok, n, H = lm.generate_code(g["proto"], table, 8, 7, 100000, stream)
        at += n
        assert ok and codes[k].tolist() == H.tolist() and index[k] == at - 1
    assert tested == at and words_after(s1, p1) == stream.fingerprint()


def random_cases():
    rng = np.random.RandomState(2030)
    out = []
    while len(out) < 36:
        rh, nh = int(rng.randint(3, 7)), int(rng.randint(6, 13))
        proto = (rng.rand(rh, nh) < 0.5).astype(np.int16)
        proto[rng.rand(rh, nh) < 0.08] = 2 + int(rng.randint(0, 3))   # fixed edges, any value other than 0 and 1
        if (proto > 0).sum() < 4:
            continue
        out.append((proto, int(rng.choice([6, 8])), int(rng.choice([2, 3, 7, 64, 126])), int(rng.randint(1, 1 << 20))))
    return out


@pytest.mark.parametrize("case", range(36))
def test_random_protographs_equal_the_model(L, torch, case):
    proto, g, M, seed = random_cases()[case]
    A, K = 3000, 3
    table = L.label_equations(proto, g)
    stream = lm.Stream(seed=seed)
    state, pos = stream.state()
    codes, index, tested, tree_girth, (s1, p1) = L.label_codes(proto, g, M, A, state, pos, want=K)
    assert tree_girth == table["tree_girth"]
    got, at, left = [], 0, A
    idx = []
    while left > 0 and len(got) < K:
        ok, n, H = lm.generate_code(proto, table, g, M, left, stream)
        if n == 0:
            break
        left -= n
        at += n
        if ok:
            got.append(H.tolist())
            idx.append(at - 1)
    print(case, proto.shape, g, M, table["n_equations"], table["n_random"], table["never_accepts"], len(got), tested)
    assert codes.tolist() == got and index.tolist() == idx and tested == at
    assert words_after(s1, p1) == stream.fingerprint()


def test_accepted_appendix_c_labellings_have_the_girth(L, torch):
    """The cross-check between two independent implementations: what passed the equations for girth g has no cycle below g under
    the girth trace (ldpc_hip_girth_codes)."""
    for name in ("appc_g6_m126", "appc_g8_m399"):
        g = GOLDENS[name]
        state, pos = lm.Stream(seed=g["seed"]).state()
        codes, _, _, _, _ = L.label_codes(g["proto"], g["target_girth"], g["M"], g["max_attempts"], state, pos, want=len(g["calls"]))
        assert len(codes) == len(g["calls"])
        S, SA, _ = L.girth_codes(codes, g["M"])
        for s, sa in zip(S, SA):
            girth = L.trace_matrix(s, sa)[0]
            print(name, girth)
            assert girth >= g["target_girth"]


def test_cpp_layer(L, torch, tmp_path):
    """reset_random; ldpc::generate_code twice; ldpc::next_random_int: upstream's loop on the library's generator, against the golden
    of the same sequence; also a protograph that does not allow the girth (no draw) and a stream with a redraw."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "label_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "label_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    for name in ("appc_g6_m126_two_calls", "k23_g14_m50", "small_redraw_seed531"):
        g = GOLDENS[name]
        calls = len(g["calls"])
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([*g["proto"].shape, g["target_girth"], g["M"], g["max_attempts"], g["seed"], calls], dtype=np.int32).tobytes())
            f.write(g["proto"].astype(np.int32).tobytes())
        out = subprocess.check_output([exe, str(tmp_path / "in.bin")], timeout=120).decode().strip().split("\n")
        for k, call in enumerate(g["calls"]):
            words = out[k].split()
            assert words[0] == "call" and int(words[1]) == int(call["ok"]), (name, k)
            if call["ok"]:
                assert [int(v) for v in words[2:]] == np.array(call["matrix"]).reshape(-1).tolist(), (name, k)
        assert [int(v) for v in out[calls].split()[1:]] == g["fingerprint"], name
