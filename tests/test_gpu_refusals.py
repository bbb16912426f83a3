"""What ldpc_hip_open answers for a single code that no tier serves, word for word, and which tier it picks for a shape every tier
takes.  The texts are the library's from before its decoders were described by decoder_kinds[] (ldpc_hip.hip); nothing here
compiles with hiprtc."""
import numpy as np
import pytest

from ldpc_testlib import ASP_DEC, IASP_DEC, LCHE_DEC, MS_DEC, TASP_DEC

pytestmark = pytest.mark.gpu

# 2 x 3 at M = 4: every block column used, the second block row of weight 1
H_ROW_WEIGHT_1 = np.array([[0, 1, 2], [-1, -1, 3]], dtype=np.int16)

NO_TIER = ("ldpc_hip_open: decoder %d, code 2x3 lifting 4: not supported by the generic kernel (limits: 16 block rows, 32 block columns, "
           "row weight 16, M <= 512, 160 KiB LDS), no code-specialised instance: this code shape has no code-specialised kernel; "
           "the shape-unlimited tier serves every built decoder; decoders 2, 5 and 7 need row weights >= 2, decoder 9 row weights <= 1024 "
           "(code -2)")


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ldpc_lib_amd
    return ldpc_lib_amd


@pytest.mark.parametrize("dec_id", [ASP_DEC, IASP_DEC, TASP_DEC])
def test_row_weight_one_is_refused_by_every_tier(L, dec_id):
    """map_bin and imap_bin read SB[1]: no tier of decoders 2, 5 and 7 takes a row of weight 1 (LDPC_HIP_EUNSUPPORTED)"""
    with pytest.raises(L.LdpcHipError) as e:
        L.LdpcHip(dec_id, H_ROW_WEIGHT_1, 4)
    assert str(e.value) == NO_TIER % dec_id


def test_lche_row_weight_limit(L):
    with pytest.raises(L.LdpcHipError) as e:
        L.LdpcHip(LCHE_DEC, np.zeros((1, 1025), dtype=np.int16), 1)
    assert str(e.value) == ("ldpc_hip_open: LCHE_DEC: row weight 1025, at most 1024 is supported (upstream's map_bin_llr overflows beyond) "
                            "(code -2)")


@pytest.mark.parametrize("env,kernel", [("LDPC_HIP_MS_VARIANT=-1", "ms_flood_kernel"), ("LDPC_HIP_FORCE_GLOBAL=1", "ms_global_kernel")])
def test_min_sum_opens_the_same_matrix_on_the_tier_asked_for(L, monkeypatch, env, kernel):
    import torch
    monkeypatch.setenv(*env.split("="))
    with L.LdpcHip(MS_DEC, H_ROW_WEIGHT_1, 4) as dec:
        assert dec.kernel_name == kernel
        dec.decode(torch.ones(3, dec.N, dtype=torch.float64, device="cuda"), 2)
        torch.cuda.synchronize()
        assert dec.last_launch() == kernel
