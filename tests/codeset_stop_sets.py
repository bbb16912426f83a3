"""Inputs of the device stopping-rule tests (test_codeset_stop_cpu.py, test_gpu_codeset_stop.py): code sets whose code 0 is the
all-weight-1 matrix of test_stopping_rule_from_cpp, the batch schedule of ldpc_hip_simulate_codes_stop restated, and the run
parameters per case.  Constants only: nothing is searched at test time."""
import numpy as np

from ldpc_testlib import LMS_DEC, MS_DEC, random_qc_code

TASP_DEC = 7
MAXITER = 20
RH, NH = 4, 8
PIECE_CAP = 1 << 16   # frames per piece of the simulate entry points when neither the 1 GiB bound nor LDPC_HIP_CODES_PIECE cuts it

# name -> decoder, M, SNR [dB], seed, n_frame_errors, n_experiments, reference_frame_error.  ms_M32 carries the inputs of
# test_stopping_rule_from_cpp (seed 9 as its in.bin); the others keep its budget and differ in decoder, lifting and SNR.
CASES = {
    "ms_M32": (MS_DEC, 32, 4.0, 9, 12, 1500, 0.05),
    "lms_M32": (LMS_DEC, 32, 4.0, 9, 12, 1500, 0.05),
    "tdmp_M32": (TASP_DEC, 32, 4.0, 9, 12, 1500, 0.05),
    "ms_M20": (MS_DEC, 20, 4.0, 9, 12, 1500, 0.05),
    "lms_M20": (LMS_DEC, 20, 4.0, 9, 12, 1500, 0.05),
    "tdmp_M20": (TASP_DEC, 20, 4.0, 9, 12, 1500, 0.05),
    "ms_M126": (MS_DEC, 126, 5.0, 9, 12, 1500, 0.05),
    "lms_M126": (LMS_DEC, 126, 5.0, 9, 12, 1500, 0.05),
    "tdmp_M126": (TASP_DEC, 126, 5.0, 9, 12, 1500, 0.05),
}


def code_set(M, ncodes=4):
    """[weak, medium, strong, medium'][:ncodes] at lifting M: code 0 has every block column of weight 1 (no coding gain, two
    circulants per block row), so it stops first and slot 0 of every later launch is code 1."""
    rng = np.random.RandomState(5)
    strong = random_qc_code(rng, RH, NH, M, [3])
    medium = random_qc_code(rng, RH, NH, M, [2])
    other = random_qc_code(rng, RH, NH, M, [2, 3])
    weak = -np.ones((RH, NH), dtype=np.int16)
    for k in range(NH):
        weak[k % RH, k] = k % M
    return np.array([weak, medium, strong, other][:ncodes], dtype=np.int16)


def schedule(n_experiments, first_batch, max_batch, piece=PIECE_CAP):
    """The sizes of the pieces of a run that nothing stops early, in launch order, as (batch index, frames): batches of first_batch,
    times 4 up to max_batch, capped by n_experiments + 1 - frames so far, each cut into pieces of at most `piece` frames."""
    piece = min(piece, max_batch, n_experiments + 1)
    out, first, batch, index = [], 0, first_batch, 0
    while n_experiments + 1 - first > 0:
        B = min(batch, n_experiments + 1 - first)
        for done in range(0, B, piece):
            out.append((index, min(piece, B - done)))
        first += B
        index += 1
        if batch < max_batch:
            batch = min(batch * 4, max_batch)
    return out


def stop_piece(experiment, pieces):
    """Index of the piece that holds the last frame a code consumed (frame number `experiment`, counted from 1): the rule runs after
    every piece, so this is the last piece launched for the code."""
    seen = 0
    for i, (_, n) in enumerate(pieces):
        seen += n
        if experiment <= seen:
            return i
    raise AssertionError((experiment, seen))


def frames_launched(experiment, pieces):
    return sum(n for _, n in pieces[:stop_piece(experiment, pieces) + 1])
