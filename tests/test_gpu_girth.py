"""Girth / ACE trace on the GPU (ldpc_hip_girth_codes, csrc/ldpc_girth.hpp): every golden case of the compiled reference
(tests/golden/girth/), random sets against the numpy restatement (tests/girth_model.py), a set against its codes one by one, pieces,
the C++ layer (include/ldpc/girth.h) and `ldpc_sim --girth`.  Everything is integer: array_equal throughout."""
import os
import re
import subprocess

import numpy as np
import pytest

import girth_model as gm
from ldpc_testlib import MS_DEC, ROOT

pytestmark = pytest.mark.gpu

GOLDENS = gm.load_goldens()


@pytest.fixture(scope="module")
def L():
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def run_golden(L, g, codes=None):
    return L.girth_codes(g["codes"] if codes is None else codes, g["M"], gmax=g["gmax"], gtarget=g["gtarget"], min_ace=g["min_ace"], max_spec=g["max_spec"])


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_girth_codes_equals_golden(L, torch, name):
    g = GOLDENS[name]
    S, SA, status = run_golden(L, g)
    print(name, S.tolist(), SA.tolist(), status.tolist())
    assert np.array_equal(S, g["S"]) and np.array_equal(SA, g["SA"])
    assert np.array_equal(status, g["ret"]), "bit 0 = upstream's return value, bit 1 (overflow) clear"


def random_set(seed, rh, nh, M, C):
    """C codes of one shape with a mask and shifts of their own: edge counts differ, columns of weight 0 and 1 occur."""
    rng = np.random.RandomState(seed)
    codes = np.where(rng.rand(C, rh, nh) < 0.45, rng.randint(0, M, (C, rh, nh)), -1)
    codes[0] = -1            # a code without any edge: nothing to trace, upstream returns 1
    codes[1][:, 0] = 0       # a full column
    return codes.astype(np.int16)


_MODEL = {}


def model_set(key):
    """Once per set: the codes, the bounds and the model's results."""
    if key not in _MODEL:
        seed, rh, nh, M, bounds = key
        codes = random_set(seed, rh, nh, M, 33)
        mn, mx = (None, None) if not bounds else ([5] * 20, [0] * 20)
        want = [gm.trace(hd, M, 20, 4, mn, mx) for hd in codes]
        assert max(w[3] for w in want) < 2 ** 31
        _MODEL[key] = (codes, mn, mx, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), np.array([w[2] for w in want]))
    return _MODEL[key]


RANDOM_SETS = [(11, 3, 6, 7, True), (12, 4, 8, 16, True), (13, 8, 16, 5, True), (14, 5, 9, 1, False)]


@pytest.mark.parametrize("key", RANDOM_SETS, ids=lambda k: "seed%d_%dx%d_M%d" % k[:4])
def test_random_sets_equal_the_model(L, torch, key):
    codes, mn, mx, S, SA, ret = model_set(key)
    got = L.girth_codes(codes, key[3], min_ace=mn, max_spec=mx)
    assert np.array_equal(got[0], S) and np.array_equal(got[1], SA) and np.array_equal(got[2], ret)
    assert (set(ret.tolist()) == {0, 1} or key[0] == 13) and len({int((c >= 0).sum()) for c in codes}) > 5


def test_a_set_equals_its_codes_one_by_one(L, torch):
    for name in ("set_one_mask", "set_two_masks"):
        g = GOLDENS[name]
        S, SA, status = run_golden(L, g)
        for c in range(len(g["codes"])):
            s, sa, st = run_golden(L, g, g["codes"][c])
            assert np.array_equal(s[0], S[c]) and np.array_equal(sa[0], SA[c]) and st[0] == status[c], (name, c)
    codes, mn, mx, S, SA, ret = model_set(RANDOM_SETS[1])
    for c in (0, 1, 7, 32):
        s, sa, st = L.girth_codes(codes[c], 16, min_ace=mn, max_spec=mx)
        assert np.array_equal(s[0], S[c]) and np.array_equal(sa[0], SA[c]) and st[0] == ret[c], c


@pytest.mark.parametrize("piece", ["1", "5", "64"])
def test_pieces_give_identical_output(L, torch, monkeypatch, piece):
    """LDPC_HIP_GIRTH_PIECE is read per call: 33 codes in pieces of 1, of 5 (a short last piece) and in one piece."""
    codes, mn, mx, S, SA, ret = model_set(RANDOM_SETS[1])
    monkeypatch.setenv("LDPC_HIP_GIRTH_PIECE", piece)
    got = L.girth_codes(codes, 16, min_ace=mn, max_spec=mx)
    monkeypatch.delenv("LDPC_HIP_GIRTH_PIECE")
    default = L.girth_codes(codes, 16, min_ace=mn, max_spec=mx)
    for a, b, want in zip(got, default, (S, SA, ret)):
        assert np.array_equal(a, b) and np.array_equal(a, want)


def test_overflow_sets_the_status_bit_and_the_other_codes_are_untouched(L, torch):
    """All-zero shifts at M = 1 on a dense 6 x 8 matrix: the walk counts pass 2^31 within the 9 steps (the model's int64 peak says
    so).  The dense code reports bit 1; the golden code beside it in the same set keeps its result."""
    dense = np.zeros((6, 8), dtype=np.int16)
    peak = gm.trace(dense, 1, 20, 20, [0] * 20, None)[3]
    assert peak >= 2 ** 31
    other = np.full((6, 8), -1, dtype=np.int16)
    other[:3, :4] = 0
    want = gm.trace(other, 1, 20, 20, [0] * 20, None)
    assert want[3] < 2 ** 31
    S, SA, status = L.girth_codes(np.stack([dense, other]), 1, gtarget=20, min_ace=[0] * 20)
    assert status[0] & 2 and status[1] == want[2]
    assert np.array_equal(S[1], want[0]) and np.array_equal(SA[1], want[1])


def test_cpp_layer(L, torch, tmp_path):
    """ldpc::trace_matrix per code, ldpc::trace_matrices on the vector, and the ggp variant's signed girth under bounds, through a
    compiled program, on the golden set whose codes stop at different depths."""
    L.load_library()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    exe = str(tmp_path / "girth_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "girth_driver.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "ldpc-lib_amd"), "-lldpc_compat", "-lldpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "ldpc-lib_amd")])
    g = GOLDENS["set_one_mask"]
    codes = g["codes"]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(codes), codes.shape[1], codes.shape[2], g["M"]], dtype=np.int32).tobytes())
        f.write(np.array(g["min_ace"] + [-1] * 20, dtype=np.int32).tobytes())
        f.write(codes.astype(np.int32).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin")], timeout=120).decode().split("\n")
    rows = {(w[0], int(w[1])): [int(v) for v in w[2:]] for w in (line.split() for line in out if line)}
    assert len(rows) == 3 * len(codes), out
    for c, hd in enumerate(codes):
        S, SA, _, _ = gm.trace(hd, g["M"], 20, 4, [0] * 20, [100000000] * 20)       # main_simulation.cpp:162-163
        girth, ace, spec = gm.trace_matrix(S, SA)
        assert rows["one", c] == rows["set", c] == [girth] + ace + spec, c
        girth, ace, spec = gm.trace_matrix(g["S"][c], g["SA"][c])
        assert rows["bounded", c] == [girth if g["ret"][c] else -girth] + ace + spec, c
    assert {rows["bounded", c][0] > 0 for c in range(len(codes))} == {True, False}


# ---- ldpc_sim --girth ---------------------------------------------------------------------------------------------------------------
def code_record(H, M, q_mod=2):
    rows = "\n".join("        " + " ".join("%4d" % v for v in row) for row in H)
    coef = "" if q_mod == 2 else "      coef = matrix (%d %d) {\n%s\n      }\n" % (H.shape[0], H.shape[1], "\n".join(
        "        " + " ".join("%4d" % (1 if v >= 0 else -1) for v in row) for row in H))
    return """    {
      _SNRs = array { 3 3.5 }
      _decoder_type = %d
      _iterations = 10
      _lifting = %d
      _q_mod = %d
      _marking = "skip"
      _punctured_blocks = 0
      code = matrix (%d %d) {
%s
      }
%s      girth = 6
      config_index = 1
    }""" % (MS_DEC, M, q_mod, H.shape[0], H.shape[1], rows, coef)


def run_sim(tmp_path, records, tag, *flags):
    scenario = tmp_path / "scenario.jsonx"
    scenario.write_text("""{
  settings = {
    random_seed = 3
    num_codewords = 40
    error_blocks = 1000000
    error_minimization = { name = "FER" threshold = 1 good_code_multiple = 1.25 }
    modulation_type = 0
    permutation_type = 0
    permutation_block = 128
    permutation_inter = 1
  }
  results = array {
%s
  }
}""" % "\n".join(records))
    exe = os.path.join(ROOT, "ldpc-lib_amd", "ldpc_sim")
    out = tmp_path / (tag + ".jsonx")
    run = subprocess.run([exe, "simulation", str(scenario), str(out), *flags], capture_output=True, text=True, timeout=120, env=dict(os.environ, LDPC_HIP_JIT="0"))
    assert run.returncode == 0, run.stderr
    return re.sub(r"\btime = \S+", "time = -", out.read_text()), run.stdout


GIRTH_FIELDS = r"\n *girth_ = \S+\n *girth_ACE = array \{[^}]*\}\n *girth_spectrum = array \{[^}]*\}"


@pytest.mark.parametrize("M", [126, 64])
def test_ldpc_sim_girth_writes_the_golden_fields(L, torch, tmp_path, M):
    """Two 16 x 32 codes: with --girth every record holds upstream's girth_, girth_ACE and girth_spectrum right behind `girth`, with
    and without --code-sets (one trace call for the group); without the flag the file is the same text less those three fields."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    g = GOLDENS["sim_pair_m%d" % M]
    records = [code_record(H, M) for H in g["codes"]]
    base, _ = run_sim(tmp_path, records, "base")
    plain, _ = run_sim(tmp_path, records, "girth", "--girth")
    sets, log = run_sim(tmp_path, records, "sets", "--girth", "--code-sets")
    assert "set of 2 codes" in log and sets == plain
    assert "girth_" not in base and re.sub(GIRTH_FIELDS, "", plain) == base
    found = re.findall(r"girth = 6\n *girth_ = (\d+)\n *girth_ACE = array \{([^}]*)\}\n *girth_spectrum = array \{([^}]*)\}\n *config_index = 1", plain)
    assert len(found) == 2
    for c, (girth, ace, spec) in enumerate(found):
        assert (int(girth), [int(v) for v in ace.split()], [int(v) for v in spec.split()]) == gm.trace_matrix(g["S"][c], g["SA"][c]), c


def test_ldpc_sim_girth_writes_zeros_for_a_code_over_gfq(L, torch, tmp_path):
    """_q_mod > 2: upstream traces nothing (main_simulation.cpp:494-498): girth_ = 0 and four zeros twice."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "ldpc-lib_amd", "csrc", "compat")])
    H = GOLDENS["gf16_m8"]["codes"][0]
    text, _ = run_sim(tmp_path, [code_record(H, 8, q_mod=16)], "gfq", "--girth")
    assert re.search(r"girth_ = 0\n *girth_ACE = array \{ 0 0 0 0 \}\n *girth_spectrum = array \{ 0 0 0 0 \}", text), text
