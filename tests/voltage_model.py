"""numpy restatement of upstream's equation_builder::check_voltages / check_voltages_and_coefs (equations.cpp:150-267) and of the loop
of random_search_bank_good_codes behind the equation table of ldpc_hip_label_equations_host, with the status 2 that
ldpc_hip_check_voltages defines where upstream exits.  The goldens (tests/golden/voltage/, tools/make_voltage_goldens.py) hold what
the compiled upstream sources gave; the draws are those of tests/label_model.py."""
import json
import os

import numpy as np

import label_model as lm

VOLTAGE_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voltage")


def golden_path(kind):
    return os.path.join(VOLTAGE_GOLDEN_DIR, kind + ".json")


def load_golden(kind):
    """check.json or bank.json as it is: case name -> upstream's results (tools/make_voltage_goldens.py: goldens() joins them with the inputs)"""
    with open(golden_path(kind)) as f:
        return json.load(f)


def all_random(proto):
    """every edge counted as random: the protograph the voltage check builds its equations on"""
    return (np.asarray(proto) > 0).astype(np.int16)


def divisors(s):
    d = np.arange(1, int(np.sqrt(s)) + 2, dtype=np.int64)
    d = d[(d * d <= s) & (s % d == 0)]
    return np.union1d(d, s // d)


def reduce(failed, max_modulo):
    """(min_ok, max_nonok) of a set of failed moduli, all <= max_modulo"""
    members = set(int(m) for m in failed)
    m = 2
    while m in members:
        m += 1
    return m, (max(members) if members else 1)


def check_voltages(table, voltages, max_modulo, coefs=None):
    """table: label_equations(all_random(proto), g).  A list of dicts per labelling: status, min_ok, max_nonok, max_abs_sum, failed
    (ascending list); min_ok = max_nonok = 0 and failed = [] for status 1."""
    eq = lm.dense_table(table)
    V = np.atleast_2d(np.asarray(voltages, dtype=np.int64))
    S = np.rint(V.astype(np.float64) @ eq.T).astype(np.int64).reshape(len(V), table["n_equations"])
    Cs = None if coefs is None else np.rint(np.atleast_2d(np.asarray(coefs)).astype(np.float64) @ eq.T).astype(np.int64).reshape(S.shape)
    out = []
    for k in range(len(V)):
        zero = S[k] == 0
        rescued = zero & (Cs[k] != 0) if Cs is not None else np.zeros_like(zero)
        status = 1 if (zero & ~rescued).any() else 2 if rescued.any() else 0
        r = {"status": status, "max_abs_sum": int(np.abs(S[k]).max()) if S.shape[1] else 0, "min_ok": 0, "max_nonok": 0, "failed": []}
        if status != 1:
            failed = set()
            for s in np.unique(np.abs(S[k][~zero])):
                failed.update(int(d) for d in divisors(int(s)) if d <= max_modulo)
            r["failed"] = sorted(failed)
            r["min_ok"], r["max_nonok"] = reduce(failed, max_modulo)
        out.append(r)
    return out


def check_modulo(r, m):
    return r["status"] == 0 and m >= r["min_ok"] and (m > r["max_nonok"] or m not in r["failed"])


def bank(proto, table, T, exact_modulo, max_attempts, want, stream):
    """The bank loop with a budget.  table: label_equations(proto, g) -- over the random edges; the fixed ones are 0 and drop out.
    Returns (accepted [(attempt index, min_ok, matrix)], attempts tested); the stream ends behind the last draw of the want-th accepted
    attempt or behind all max_attempts."""
    Er = table["n_random"]
    eq = lm.dense_table(table)
    got, tested, chunk = [], 0, 64
    bound = max(T, exact_modulo)
    while tested < max_attempts and len(got) < want:
        n = min(chunk, max_attempts - tested)
        need = n * Er
        words = need + 64
        while True:
            vals, where = lm.draws(stream.peek(words), T)
            if len(vals) >= need:
                break
            words += 64
        V = vals[:need].reshape(n, Er)
        S = np.rint(V.astype(np.float64) @ eq.T).astype(np.int64).reshape(n, table["n_equations"])
        end = None
        for a in np.flatnonzero((S != 0).all(axis=1)):
            r = check_voltages(table, V[a], bound)[0]
            if r["status"] == 0 and r["min_ok"] <= T and (exact_modulo == 0 or check_modulo(r, exact_modulo)):
                got.append((tested + int(a), r["min_ok"], lm.matrix_of(proto, V[a])))
                if len(got) == want:
                    end = int(a)
                    break
        if end is not None:
            stream.advance(int(where[(end + 1) * Er - 1]) + 1 if Er else 0)
            return got, tested + end + 1
        stream.advance(int(where[need - 1]) + 1 if Er else 0)
        tested += n
        chunk = min(chunk * 4, 4096)
    return got, tested
