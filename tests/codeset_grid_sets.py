"""Inputs of the SNR-grid tests (test_codeset_grid_cpu.py, test_gpu_codeset_grid.py).  Constants only: nothing is searched at test time.
The code sets are those of codeset_stop_sets (4 x 8 base matrices, 4 codes, code 0 without coding gain) and, for the wide route, the
smallest set of codeset_wide_sets with more than 16 block rows."""
from ldpc_testlib import LMS_DEC, MS_DEC

SP_DEC, ASP_DEC, IMS_DEC, IASP_DEC, TASP_DEC, LCHE_DEC = 1, 2, 4, 5, 7, 9
DECS = {"ms": MS_DEC, "lms": LMS_DEC, "tdmp": TASP_DEC, "iasp": IASP_DEC, "lche": LCHE_DEC, "ims": IMS_DEC, "sp": SP_DEC, "asp": ASP_DEC}
SEED = 9              # std::mt19937(SEED), and the Philox seed
MAX_POINTS = 64

# 1. records: B frames at three unsorted points; liftings with three frames per wave, two, one, and two waves per frame
RECORD_FRAMES = 37
RECORD_POINTS = (3.0, 1.1, 2.5)
RECORD_LIFTINGS = (20, 32, 64, 126)
PIECE = 16            # LDPC_HIP_CODES_PIECE: pieces of 16, 16 and 5 frames

# 2. routes
WIDE_SET = "rows17_M20"            # codeset_wide_sets: 17 block rows, M = 20
WIDE_POINTS = {MS_DEC: (2.5, 1.0, 3.5), TASP_DEC: (1.0, 2.5, 0.5), LMS_DEC: (1.5, 3.0, 0.5)}
GLOBAL_LIFTINGS = (20, 64)
GLOBAL_GRID = 3                    # LDPC_HIP_CODES_GLOBAL_GRID: three workgroups walk 3 x 4 x 37 items

# 4. the rule.  M = 32, shared n_frame_errors and n_experiments, a reference frame error per point.  Chosen with the CPU oracle
# (orc_bp_simulation, seed 9) so that among the twelve (point, code) items runs end in all three ways; (experiment, nde) per code:
#   MS_DEC    3.5 dB, 1.0 : (12, 12) (214, 12) (301, 4) (214, 12)      n_frame_errors, and n_experiments for the strong code
#             1.1 dB, 0.02: (10, 10) (12, 10) (13, 10) (12, 10)        the FER rule
#             2.5 dB, 1.0 : (12, 12) (68, 12) (167, 12) (74, 12)       n_frame_errors
#   TASP_DEC  3.5 dB, 1.0 : (17, 12) (293, 12) (301, 2) (301, 10)
#             1.1 dB, 0.02: (10, 10) (12, 10) (18, 10) (13, 10)
#             2.5 dB, 1.0 : (12, 12) (82, 12) (180, 12) (105, 12)
RULE_LIFTING = 32
RULE_POINTS = (3.5, 1.1, 2.5)
RULE_REFERENCES = (1.0, 0.02, 1.0)
RULE_FRAME_ERRORS, RULE_EXPERIMENTS = 12, 300
RULE_BATCHES = (64, 256)           # first_batch, max_batch
RULE_DECS = {"ms": MS_DEC, "tdmp": TASP_DEC}


def ending(state_row, n_frame_errors=RULE_FRAME_ERRORS, n_experiments=RULE_EXPERIMENTS):
    """How a run ended, from its experiment and nde (state[0], state[2])"""
    experiment, nde = int(state_row[0]), int(state_row[2])
    if nde >= n_frame_errors:
        return "frame_errors"
    if experiment > n_experiments:
        return "experiments"
    assert nde >= 10, state_row
    return "fer_rule"
