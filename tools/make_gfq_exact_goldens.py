#!/usr/bin/env python3
"""Golden records of upstream's q-ary frame loop: tests/golden/gfq_exact/*.npz, inputs and expected outputs only.

Run where oracle/_ref exists (`make -C oracle ref` with the upstream tree mounted), so that the decoder inside the loop is the
compiled upstream:

    python3 tools/make_gfq_exact_goldens.py

Per case of tests/gfq_harness_model.py:CASES: the harness inputs (q_bits, M, H, coef, ncols2convert), what the set-up makes of them
(hb, hc, coef_back), the transmitted word, snr / punctured_blocks / maxiter / seed, the per-frame frame_info and iters, the five
counters, and under the case's stopping rule the state (experiment, nse, nde), the ending and (BER, FER).  The Gaussians are not
stored: they are the stream of std::mt19937(seed), which the oracle regenerates.

Checked before anything is written: max |LH| < 512 (beyond it glibc's exp takes a path nobody restates), every run holds errored and
clean frames, the three endings of the stopping rule all occur, the "enc" cases of S2 / S3 really encode and the shipped code really
falls back to the all-zero word, and the numpy decoder model agrees with the compiled one on every record.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gfq_harness_model as hm  # noqa: E402
from gfq_model import GfqModel  # noqa: E402


def check_inputs(sets):
    """The conditions on the inputs; sets: name -> dict / npz of a case.  Shared with the tests."""
    endings = set()
    for name, g in sets.items():
        assert float(g["max_lh"]) < 512, (name, float(g["max_lh"]))
        bad = np.asarray(g["frame_info"]) != 0
        assert bad.any() and not bad.all(), name
        endings.add(str(g["ending"]))
        assert int(g["encoded"]) == (hm.CASES[name]["word"] == "enc" and hm.CASES[name]["code"] != "shipped"), name
        assert np.asarray(g["word"]).any() == bool(int(g["encoded"])), name
    assert endings >= {"nde", "experiments", "reference"}, endings
    assert any(int(g["ncols2convert"]) > 0 for g in sets.values())


def main():
    assert hm.gfq_ref_available(), "needs oracle/_ref"
    os.makedirs(hm.EXACT_GOLDEN_DIR, exist_ok=True)
    sets = {name: hm.run_case(name) for name in hm.CASES}
    check_inputs(sets)
    for name, g in sets.items():
        p = hm.CASES[name]
        noise = hm.gaussians(p["seed"], p["frames"], g["hb"].shape[1] * p["M"] * p["q_bits"])
        soft = hm.cm.channel(p["q_bits"], np.broadcast_to(g["word"], (p["frames"], g["word"].shape[0])), noise,
                             hm.sigma_of(*g["hb"].shape, p["snr"], p["punct"]))
        iters = GfqModel(p["q_bits"], g["hb"], g["hc"], p["M"]).decode(soft, p["maxiter"])[0]
        assert np.array_equal(iters, g["iters"]), name
        path = os.path.join(hm.EXACT_GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **g)
        print(name, os.path.getsize(path), g["counters"].tolist(), g["stop_state"].tolist(), g["ending"])


if __name__ == "__main__":
    main()
