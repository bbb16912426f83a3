"""The labelling search without a GPU: the equation table of ldpc_hip_label_equations_host against the equation counts and tree girths
the compiled upstream sources reported (tests/golden/label/, tools/make_label_goldens.py); the numpy restatement (tests/label_model.py)
on that table against every golden end to end -- attempts, matrices, generator fingerprint --; every refusal of ldpc_hip_label_codes,
which it finds before any device call; the exports; the C++ header; the host enumeration under the address and undefined-behaviour
sanitizers as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import label_model as lm
from ldpc_testlib import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_label_goldens  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
GOLDENS = lm.load_goldens()


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


def test_golden_cases_are_the_tools_and_are_small_data():
    cases = make_label_goldens.cases()
    assert set(GOLDENS) == set(cases)
    for name, (proto, g, M, A, seed, K) in cases.items():
        gold = GOLDENS[name]
        assert np.array_equal(gold["proto"], proto) and (gold["target_girth"], gold["M"], gold["max_attempts"], gold["seed"]) == (g, M, A, seed), name
        assert len(gold["calls"]) == K and len(gold["fingerprint"]) == 8, name
        assert os.path.getsize(os.path.join(lm.LABEL_GOLDEN_DIR, name + ".json")) < 8192, name


def test_golden_cases_cover_what_they_are_for():
    attempts = {n: [c["attempts"] for c in g["calls"]] for n, g in GOLDENS.items()}
    oks = {n: [c["ok"] for c in g["calls"]] for n, g in GOLDENS.items()}
    assert [GOLDENS["small_g%d_m7" % g]["eqs"] for g in (6, 8, 10)] == [3, 11, 20]
    assert attempts["small_g10_m7"] == [100000] * 3 and not any(oks["small_g10_m7"])
    assert GOLDENS["k23_g12_m50"]["eqs"] == 9 and attempts["k23_g12_m50"] == [1]
    for g in (14, 16):   # the tree allows 12: false, and no draw (the fingerprint is the fresh generator's)
        gold = GOLDENS["k23_g%d_m50" % g]
        assert attempts["k23_g%d_m50" % g] == [0] and gold["eqs"] is None and gold["fingerprint"] == lm.Stream(seed=1).fingerprint()
    assert GOLDENS["same_columns_m3"]["eqs"] == 0 and attempts["same_columns_m3"][5] == 2
    assert attempts["redraw_seed357"] == [1000] and attempts["redraw_seed105"] == [2000]
    assert (1 << 32) % 32513 == 32509
    assert lm.redraw_positions(lm.Stream(seed=357).peek(4001), 32513).tolist() == [776]
    assert GOLDENS["redraw_seed357"]["fingerprint"][0] == int(lm.Stream(seed=357).peek(4002)[4001]) >> 2 == 21485204
    assert lm.redraw_positions(lm.Stream(seed=105).peek(8002), 32513).tolist() == [4165, 6644]
    for seed, word in ((531, 6), (1298, 33)):   # a redraw in front of the last accept of the 3 x 6 cases (12 draws per attempt)
        gold = GOLDENS["small_redraw_seed%d" % seed]
        assert lm.redraw_positions(lm.Stream(seed=seed).peek(12 * len(gold["calls"])), 32513).tolist() == [word] and all(oks["small_redraw_seed%d" % seed])
    appc = GOLDENS["appc_g6_m126"]["proto"]
    assert int((appc > 0).sum()) == 112 and int((appc == 2).sum()) == 32
    assert GOLDENS["appc_g6_m126"]["eqs"] == 343 and attempts["appc_g6_m126"][0] == 43
    assert GOLDENS["appc_g8_m399"]["eqs"] == 5200 and attempts["appc_g8_m399"] == [238688]
    assert attempts["appc_g8_m126_a2000"] == [2000] and not any(oks["appc_g8_m126_a2000"])


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_equation_table_equals_golden_counts(L, name):
    g = GOLDENS[name]
    t = L.label_equations(g["proto"], g["target_girth"])
    if g["eqs"] is None:
        assert t["tree_girth"] < g["target_girth"]
    else:
        assert (t["n_equations"], t["tree_girth"]) == (g["eqs"], g["tree_girth"])
    rows, cols, random = lm.layout(g["proto"])
    assert t["n_random"] == int(random.sum())
    assert t["eq_begin"][0] == 0 and t["eq_begin"][-1] == len(t["term_edge"]) == len(t["term_mult"]) and np.all(np.diff(t["eq_begin"]) >= 0)
    assert np.all(t["term_mult"] != 0) and np.all((t["term_edge"] >= 0) & (t["term_edge"] < max(t["n_random"], 1)))
    assert t["never_accepts"] == bool(np.any(np.diff(t["eq_begin"]) == 0))
    assert np.all(np.diff(np.diff(t["eq_begin"])) >= 0), "short equations first"


def test_equation_table_of_a_single_cycle_and_of_fixed_edges(L):
    """A 2 x 2 cycle: one equation v0 - v1 - v2 + v3 (up to sign) at g = 6; with every edge fixed it has no term left; with three of
    them fixed it is the one random edge alone."""
    t = L.label_equations([[1, 1], [1, 1]], 6)
    assert (t["n_equations"], t["tree_girth"], t["never_accepts"]) == (1, 6, False)
    assert sorted(zip(t["term_edge"].tolist(), (t["term_mult"] * t["term_mult"][0]).tolist())) == [(0, 1), (1, -1), (2, -1), (3, 1)]
    t = L.label_equations([[2, 3], [4, 5]], 6)
    assert (t["n_equations"], t["n_random"], t["never_accepts"], len(t["term_edge"])) == (1, 0, True, 0)
    t = L.label_equations([[2, 1], [2, 2]], 6)
    assert (t["n_equations"], t["n_random"], t["never_accepts"], t["term_edge"].tolist(), abs(t["term_mult"]).tolist()) == (1, 1, False, [0], [1])
    # g = 10 walks the cycle twice: the doubled equation is a second bag
    t = L.label_equations([[1, 1], [1, 1]], 10)
    assert t["n_equations"] == 2 and sorted(abs(t["term_mult"]).tolist()) == [1] * 4 + [2] * 4


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_model_equals_golden(L, name):
    g = GOLDENS[name]
    make_label_goldens.check_model(name, g)


def test_label_codes_refuses_bad_arguments_before_any_device_call(L):
    """Every LDPC_HIP_EINVAL of the header on a machine that may have no GPU: a call that reached the device would fail differently
    there (LDPC_HIP_EHIP), and the outputs stay untouched."""
    lib = L.load_library()
    proto = np.ascontiguousarray(GOLDENS["small_g8_m7"]["proto"])
    state = np.arange(624, dtype=np.uint32)
    hd = np.full((2, 3, 6), 77, dtype=np.int16)
    index = np.full(2, 77, dtype=np.int64)
    out = np.full(624, 77, dtype=np.uint32)
    found, tg, pos_out, tested = C.c_int(77), C.c_int(77), C.c_int(77), C.c_longlong(77)

    def call(rh=3, nh=6, proto=proto, g=8, M=7, A=100, want=2, state=state, pos=0, hd=hd, index=index, found=found, tested=tested, tg=tg, out=out,
             pos_out=pos_out):
        def ptr(a):
            return None if a is None else a.ctypes.data

        def ref(v):
            return None if v is None else C.byref(v)
        return lib.ldpc_hip_label_codes(rh, nh, ptr(proto), g, M, A, want, ptr(state), pos, 0, ptr(hd), ptr(index), ref(found), ref(tested), ref(tg),
                                        ptr(out), ref(pos_out))

    negative = proto.copy()
    negative[1, 2] = -1
    cases = {"rh 0": dict(rh=0), "nh < 0": dict(nh=-6), "proto NULL": dict(proto=None), "negative entry": dict(proto=negative),
             "no edge": dict(proto=np.zeros((3, 6), dtype=np.int16)), "girth 3": dict(g=3), "girth 0": dict(g=0), "M 1": dict(M=1), "M 0": dict(M=0),
             "M 32768": dict(M=32768), "A 0": dict(A=0), "A < 0": dict(A=-5), "want 0": dict(want=0), "want < 0": dict(want=-1),
             "state NULL": dict(state=None), "pos -1": dict(pos=-1), "pos 625": dict(pos=625), "hd NULL": dict(hd=None), "index NULL": dict(index=None),
             "found NULL": dict(found=None), "tested NULL": dict(tested=None), "tree_girth NULL": dict(tg=None), "state_out NULL": dict(out=None),
             "pos_out NULL": dict(pos_out=None)}
    for what, kw in cases.items():
        assert call(**kw) == EINVAL, what
        assert "ldpc_hip_label_codes" in lib.ldpc_hip_last_error().decode(), what
    assert "row 1, column 2: entry -1" in (call(proto=negative), lib.ldpc_hip_last_error().decode())[1]
    assert (hd == 77).all() and (index == 77).all() and (out == 77).all()
    assert (found.value, tg.value, pos_out.value, tested.value) == (77, 77, 77, 77)
    with pytest.raises(L.LdpcHipError, match="M = 40000"):
        L.label_codes(proto, 8, 40000, 10, state, 0)
    assert lib.ldpc_hip_label_equations_host(3, 6, proto.ctypes.data, 3, None, None, None, None, None, None, None, None) == EINVAL
    assert "ldpc_hip_label_equations_host" in lib.ldpc_hip_last_error().decode()


def test_label_codes_names_what_does_not_fit(L):
    """LDPC_HIP_EUNSUPPORTED, also found without a device: the equation cap (the message holds the count reached), a girth beyond 64,
    more random edges than a wave keeps in LDS."""
    state = np.arange(624, dtype=np.uint32)
    dense = np.ones((6, 12), dtype=np.int16)
    with pytest.raises(L.LdpcHipError, match=r"more than (1048576 equations|4194304 paths).*\(code -2\)"):
        L.label_equations(dense, 12)
    with pytest.raises(L.LdpcHipError, match=r"more than (1048576 equations|4194304 paths).*\(code -2\)"):
        L.label_codes(dense, 12, 64, 10, state, 0)
    with pytest.raises(L.LdpcHipError, match=r"target_girth = 66, at most 64.*\(code -2\)"):
        L.label_codes([[1, 1], [1, 1]], 66, 64, 10, state, 0)
    wide = np.zeros((2, 482), dtype=np.int16)   # a path: 481 random edges, no cycle at all
    wide[0, :] = 1
    wide[1, 0] = 2
    wide[0, 0] = 2
    with pytest.raises(L.LdpcHipError, match=r"481 edges with a random shift, at most 480.*\(code -2\)"):
        L.label_codes(wide, 4, 64, 10, state, 0)


def test_a_protograph_that_does_not_allow_the_girth_returns_without_a_device(L):
    """tree_girth < target_girth: found = 0, no attempt, the generator untouched -- decided on the host."""
    state = np.arange(624, dtype=np.uint32)
    codes, index, tested, tree_girth, (s1, p1) = L.label_codes(np.ones((2, 3), dtype=np.int16), 14, 50, 1000, state, 123)
    assert (len(codes), len(index), tested, tree_girth, p1) == (0, 0, 0, 12, 123) and np.array_equal(s1, state)


def test_exports_and_abi_version(L):
    lib = L.load_library()
    assert lib.ldpc_hip_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in ("ldpc_hip_label_equations_host", "ldpc_hip_label_codes", "ldpc_hip_label_last_stats"):
        assert hasattr(lib, name) and re.search(r"\b(int|void) %s\(" % name, header), name
    for name in ("label_equations", "label_codes", "label_last_stats"):
        assert callable(getattr(L, name)) and name in L.__all__


def test_cpp_layer_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "ldpc/code_generation.h"\n'
                   "bool f(ldpc::Matrix const &P, ldpc::Matrix &H) { return ldpc::generate_code(P, 8, 126, 1000, H); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_host_enumeration_under_sanitizers(tmp_path):
    """tests/cpp/label_sanitize.cpp: the enumeration and the table builder of csrc/ldpc_label.hpp on the goldens' protographs, compiled
    with -fsanitize=address,undefined as a program of its own; it prints equations and tree girth per protograph."""
    exe = str(tmp_path / "label_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "ldpc-lib_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "label_sanitize.cpp"), "-o", exe])
    seen = set()
    for name, g in sorted(GOLDENS.items()):
        key = (g["proto"].tobytes(), g["target_girth"])
        if key in seen:
            continue
        seen.add(key)
        words = [*g["proto"].shape, g["target_girth"], *g["proto"].reshape(-1).tolist()]
        run = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        eqs, tree_girth = (int(v) for v in run.stdout.split()[:2])
        if g["eqs"] is None:
            assert tree_girth < g["target_girth"], name
        else:
            assert (eqs, tree_girth) == (g["eqs"], g["tree_girth"]), name
