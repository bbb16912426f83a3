"""numpy restatement of upstream's generate_code (code_generation.cpp:35-115) behind the equation table of
ldpc_hip_label_equations_host: the draw filter of libstdc++'s uniform_int_distribution over std::mt19937, the divisibility predicate of
check_voltages / check_modulo, and check_same_colums.  The goldens (tests/golden/label/, tools/make_label_goldens.py) hold what the
compiled upstream sources gave."""
import glob
import json
import os

import numpy as np

LABEL_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label")


def load_goldens():
    out = {}
    for path in sorted(glob.glob(os.path.join(LABEL_GOLDEN_DIR, "*.json"))):
        with open(path) as f:
            g = json.load(f)
        g["proto"] = np.array(g["proto"], dtype=np.int16)
        out[os.path.splitext(os.path.basename(path))[0]] = g
    return out


class Stream:
    """std::mt19937: tempered 32-bit words, read ahead without being consumed."""

    def __init__(self, seed=None, state=None, pos=0):
        self.bg = np.random.MT19937()
        if state is None:
            self.bg._legacy_seeding(int(seed))   # init_genrand, as std::mt19937(seed); MT19937(seed) seeds differently
        else:
            self.bg.state = {"bit_generator": "MT19937", "state": {"key": np.asarray(state, dtype=np.uint32), "pos": int(pos)}}
        self.start = self.bg.state
        self.buf = np.zeros(0, dtype=np.uint64)   # words read ahead of the consumed ones; self.bg stands behind them
        self.consumed = 0

    def peek(self, n):
        if len(self.buf) < n:
            self.buf = np.concatenate([self.buf, self.bg.random_raw(n - len(self.buf)).astype(np.uint64)])
        return self.buf[:n]

    def advance(self, n):
        self.peek(n)
        self.buf = self.buf[n:]
        self.consumed += n
        return self

    def state(self):
        """(624 words, pos) behind the consumed words."""
        bg = np.random.MT19937()
        bg.state = self.start
        if self.consumed:
            bg.random_raw(self.consumed)
        return bg.state["state"]["key"].astype(np.uint32), int(bg.state["state"]["pos"])

    def fingerprint(self):
        """eight next_random_int(0, 1 << 30): the next words >> 2, never rejected; consumes them."""
        w = self.peek(8) >> np.uint64(2)
        self.advance(8)
        return [int(v) for v in w]


def draws(words, M):
    """(values, word index of each value): the words uniform_int_distribution<int>(0, M - 1) does not reject."""
    prod = np.asarray(words, dtype=np.uint64) * np.uint64(M)
    keep = np.flatnonzero((prod & np.uint64(0xffffffff)) >= np.uint64((1 << 32) % M))
    return (prod[keep] >> np.uint64(32)).astype(np.int64), keep


def redraw_positions(words, M):
    prod = np.asarray(words, dtype=np.uint64) * np.uint64(M)
    return np.flatnonzero((prod & np.uint64(0xffffffff)) < np.uint64((1 << 32) % M))


def layout(proto):
    """cells column by column: (rows, cols) of the edges and which of them draw."""
    proto = np.asarray(proto)
    cols, rows = np.nonzero(proto.T > 0)
    return rows, cols, proto[rows, cols] == 1


def dense_table(table):
    eq = np.zeros((table["n_equations"], table["n_random"]), dtype=np.float64)
    for i in range(table["n_equations"]):
        lo, hi = table["eq_begin"][i], table["eq_begin"][i + 1]
        np.add.at(eq[i], table["term_edge"][lo:hi], table["term_mult"][lo:hi])
    return eq


def passes(V, eq, M):
    """attempts [n, Er] -> which pass every equation: no signed sum divisible by M (an exact 0 included)."""
    alive = np.arange(len(V))
    for lo in range(0, len(eq), 256):   # most attempts die early: the survivors alone meet the later equations
        if len(alive) == 0:
            break
        sums = np.rint(V[alive].astype(np.float64) @ eq[lo:lo + 256].T).astype(np.int64)
        alive = alive[(sums % M != 0).all(axis=1)]
    ok = np.zeros(len(V), dtype=bool)
    ok[alive] = True
    return ok


def matrix_of(proto, v):
    rows, cols, random = layout(proto)
    out = np.full(np.asarray(proto).shape, -1, dtype=np.int64)
    shifts = np.zeros(len(rows), dtype=np.int64)
    shifts[random] = v
    out[rows, cols] = shifts
    return out


def same_columns(H):
    cols = [tuple(c) for c in H.T]
    return len(set(cols)) < len(cols)


def generate_code(proto, table, target_girth, M, max_attempts, stream):
    """One call of upstream's: (ok, attempts tested, result matrix or None); the stream ends where upstream's generator does."""
    if table["tree_girth"] < target_girth:
        return False, 0, None
    Er = table["n_random"]
    eq = dense_table(table)
    tested, chunk = 0, 64
    while tested < max_attempts:
        n = min(chunk, max_attempts - tested)
        need = n * Er
        words = need + 64
        while True:
            vals, where = draws(stream.peek(words), M)
            if len(vals) >= need:
                break
            words += 64
        V = vals[:need].reshape(n, Er)
        for a in np.flatnonzero(passes(V, eq, M)):
            H = matrix_of(proto, V[a])
            if not same_columns(H):
                stream.advance(int(where[(a + 1) * Er - 1]) + 1 if Er else 0)
                return True, tested + int(a) + 1, H
        stream.advance(int(where[need - 1]) + 1 if Er else 0)
        tested += n
        chunk = min(chunk * 4, 16384)
    return False, max_attempts, None
