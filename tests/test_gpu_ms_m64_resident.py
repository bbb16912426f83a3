"""GPU: ms_m64_body keeps the channel values of its first non-local block columns in LDS, and has an instance without soft values.

The frame prologue loads the first R non-local columns once and stores y + 0.0 in slots of the frame's LDS share: the spare
columns behind the image, and -- in the instance a launch without soft_out runs, ms_m64_hard_body -- the image slots of the local
columns, whose hard bits that instance shifts into bit words instead of storing their soft values (ms_m64_resident_cols,
ms_m64_resident_slot, ms_m64_local_place of ldpc_spec.hpp, restated below).  The other non-local columns keep STATE2's stream.
What can go wrong, and what this file aims at:

  - the rule's ends: no local column (R from the spare alone), every column local (R = 0), as many non-local columns as there is
    room, fewer and more (the difference is even without soft values whatever NH is, any number with them);
  - the frame's LDS share at block-column counts around its boundaries: 32 (spare 6), 36 (spare 2), 38 (spare 0), 39 (7 frames per
    CU, spare 5);
  - more than 32 local columns: two bit words.  (The codes have few block rows and, where many columns are local, few local
    columns per block row: the compile time of an instance grows quickly with those);
  - AWGN at 0 and 2 dB and the adversarial LLRs of ldpc_testlib with +-0.0 on the resident columns (the canonicalisation moved
    into the prologue), maxiter 1, 2, 3 and 50, both exits of the iteration loop;
  - every case through both instances in one context, with and without soft_out in turn: the choice is made per launch;
  - a few thousand frames through the persistent launch of the shipped instances: a wave refills its slots for its next frame.

Everything is compared with the CPU oracle bit for bit: hard decisions, signed iteration counts, soft values where requested."""
import functools

import numpy as np
import pytest

from ldpc_testlib import MS_DEC, Oracle, adversarial_llr, assert_bits_equal, awgn_llr, pack_bits
from test_gpu_ms_m64_local import AOT_NAME, _every_shift_zero, _matrix, _no_shift_zero, _shipped, _signs, local_columns

gpu = pytest.mark.gpu   # the tests that decode; those that only look at the matrices run anywhere

M = 64
FRAMES = 16
LDS_BUDGET = 160 * 1024 - 64   # kMsM64LdsBudget
FRAMES_PER_CU = 8              # kMsM64FramesPerCu


def image_bytes(nh):
    """kMsM64LdsBytes"""
    return 8 * nh * M + 512


def frame_lds_bytes(nh):
    """kMsM64FrameLdsBytes: the budget over the frames a CU holds, rounded down to whole block columns"""
    frames = min(LDS_BUDGET // image_bytes(nh), FRAMES_PER_CU)
    return max(LDS_BUDGET // frames // 512 * 512, image_bytes(nh))


def frames_per_cu(nh):
    return min(LDS_BUDGET // image_bytes(nh), FRAMES_PER_CU)


def spare_columns(nh):
    """ms_m64_spare_cols"""
    return (frame_lds_bytes(nh) - image_bytes(nh)) // 512


def nonlocal_columns(H):
    loc = local_columns(H)
    return [k for k in range(H.shape[1]) if k not in loc]


def room(H, soft):
    return spare_columns(H.shape[1]) + (0 if soft else len(local_columns(H)))


def resident_columns(H, soft):
    """ms_m64_resident_cols: how many of the non-local columns, in ascending order, are resident"""
    return min(room(H, soft), len(nonlocal_columns(H)))


def resident_slots(H, soft):
    """ms_m64_resident_slot for the resident columns: the spare slots NH, NH + 1, ... first, then the local columns' own"""
    nh = H.shape[1]
    slots = list(range(nh, nh + spare_columns(nh))) + ([] if soft else local_columns(H))
    return slots[:resident_columns(H, soft)]


def local_places(H):
    """ms_m64_local_place: local column -> its place in STATE3's order (first block row, then slot = ascending column)"""
    first = {k: int(np.flatnonzero(H[:, k] >= 0)[0]) for k in local_columns(H)}
    return {k: p for p, k in enumerate(sorted(first, key=lambda k: (first[k], k)))}


def local_bits(H):
    """ms_m64_local_bit: local column -> (word, bit) once the word's last column is shifted in"""
    places, n = local_places(H), len(local_columns(H))
    return {k: (p // 32, min(n - 32 * (p // 32), 32) - 1 - p % 32) for k, p in places.items()}


def _code(nh, nloc, rh=3):
    """rh x nh: block column k has an edge in block row k mod rh, every second one while the row weights allow (16) a second edge in
    a neighbouring block row; `nloc` columns spread over the range are local (shifts 0), the others rotated."""
    loc = {int(k) for k in np.linspace(0, nh - 1, nloc).round()} if nloc else set()
    k = 0
    while len(loc) < nloc:   # (rounding met a column twice)
        loc.add(k)
        k += 1
    entries, w = [], [0] * rh
    for k in range(nh):
        entries.append((k % rh, k, 0 if k in loc else 1 + (5 * k + 3) % 63))
        w[k % rh] += 1
    for k in range(0, nh, 2):
        j = k % rh + 1 if k % rh + 1 < rh else k % rh - 1   # (a neighbouring block row: a column of shifts 0 stays local)
        if w[j] < 16:
            entries.append((j, k, 0 if k in loc else 1 + (11 * k + 7) % 63))
            w[j] += 1
    return _matrix(rh, nh, entries)


CODES = {"no_local_column_3x6": _no_shift_zero,
         "every_column_local_2x4": _every_shift_zero,
         "nh32_spare_6": lambda: _code(32, 10),
         "nh36_more_than_room_without_soft": lambda: _code(36, 16, rh=6),
         "nh36_as_much_as_room_without_soft": lambda: _code(36, 17, rh=6),
         "nh36_less_than_room_without_soft": lambda: _code(36, 18, rh=6),
         "nh36_two_bit_words": lambda: _code(36, 33, rh=9),
         "nh20_one_more_than_room_with_soft": lambda: _code(20, 1),
         "nh20_as_much_as_room_with_soft": lambda: _code(20, 2),
         "nh20_one_less_than_room_with_soft": lambda: _code(20, 3),
         "nh38_spare_0": lambda: _code(38, 12, rh=6),
         "nh39_seven_frames_per_cu": lambda: _code(39, 12, rh=4),
         "shipped_16x32": _shipped}


def test_the_frame_share_at_the_boundaries():
    assert (LDS_BUDGET, image_bytes(32)) == (163776, 16896)
    assert {nh: (frames_per_cu(nh), spare_columns(nh)) for nh in (32, 36, 38, 39)} == {32: (8, 6), 36: (8, 2), 38: (8, 0), 39: (7, 5)}
    for nh in range(1, 65):
        assert frame_lds_bytes(nh) % 512 == 0 and frame_lds_bytes(nh) >= image_bytes(nh)
        assert frames_per_cu(nh) * frame_lds_bytes(nh) <= LDS_BUDGET      # residency never lowers the frames per CU
        assert spare_columns(nh) == (39 if nh < 39 else 45 if nh < 45 else 53 if nh < 53 else 63 if nh < 63 else 79) - 1 - nh


def test_the_matrices_hold_what_they_are_meant_to_exercise():
    got = {case: (H.shape[1], len(local_columns(H)), resident_columns(H, False), resident_columns(H, True))
           for case, H in ((case, make()) for case, make in CODES.items())}
    assert got == {"no_local_column_3x6": (6, 0, 6, 6),
                   "every_column_local_2x4": (4, 4, 0, 0),
                   "nh32_spare_6": (32, 10, 16, 6),
                   "nh36_more_than_room_without_soft": (36, 16, 18, 2),
                   "nh36_as_much_as_room_without_soft": (36, 17, 19, 2),
                   "nh36_less_than_room_without_soft": (36, 18, 18, 2),
                   "nh36_two_bit_words": (36, 33, 3, 2),
                   "nh20_one_more_than_room_with_soft": (20, 1, 19, 18),
                   "nh20_as_much_as_room_with_soft": (20, 2, 18, 18),
                   "nh20_one_less_than_room_with_soft": (20, 3, 17, 17),
                   "nh38_spare_0": (38, 12, 12, 0),
                   "nh39_seven_frames_per_cu": (39, 12, 17, 5),
                   "shipped_16x32": (32, 15, 17, 6)}, got
    for case, make in CODES.items():
        H = make()
        nl = len(nonlocal_columns(H))
        assert int((H >= 0).sum(axis=1).max()) <= 16, case
        for soft in (False, True):
            slots = resident_slots(H, soft)
            assert len(set(slots)) == len(slots) and not set(slots) & set(nonlocal_columns(H)), (case, soft)
            assert all(512 * (s + 2) <= frame_lds_bytes(H.shape[1]) for s in slots), (case, soft)   # slot s sits 512 (s + 1) B in
        bits = local_bits(H)
        assert len(set(bits.values())) == len(bits) and all(0 <= b < 32 for _, b in bits.values()), case
    H = CODES["nh36_more_than_room_without_soft"]()
    assert len(nonlocal_columns(H)) - room(H, False) == 2 and len(nonlocal_columns(H)) - room(H, True) > 8   # a stream of depth 8 is left
    assert len(nonlocal_columns(CODES["nh36_less_than_room_without_soft"]())) - room(CODES["nh36_less_than_room_without_soft"](), False) == -2
    assert max(w for w, _ in local_bits(CODES["nh36_two_bit_words"]()).values()) == 1
    for case, diff in (("nh20_one_more_than_room_with_soft", 1), ("nh20_as_much_as_room_with_soft", 0), ("nh20_one_less_than_room_with_soft", -1)):
        assert len(nonlocal_columns(CODES[case]())) - room(CODES[case](), True) == diff, case
    assert resident_slots(_shipped(), False) == [32, 33, 34, 35, 36, 37] + list(range(11)) and resident_slots(_shipped(), True) == list(range(32, 38))
    assert local_places(_shipped()) == {k: k for k in range(15)}


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """name -> LLRs [<= 2 FRAMES, N]; computed once per case"""
    H = CODES[case]()
    no = list(CODES).index(case)
    Hi = np.asarray(H, dtype=np.int32)
    rh, nh = H.shape
    N = nh * M
    adv = adversarial_llr(H, M, 110 + no)[0].copy()
    res = sorted(set(nonlocal_columns(H)[:max(resident_columns(H, False), resident_columns(H, True))]))
    for f, val in enumerate([-0.0, 0.0, -0.0, -5e-324]):
        for k in res:
            adv[f, k * M:(k + 1) * M] = val                      # the whole resident column
            adv[f + 4, k * M + (f % 2):(k + 1) * M:2] = val      # every other lane of it
    # the Es/N0 of a rate-1/2 code at Eb/N0 = 12 dB (a code of higher rate loses the difference): the first iteration's hard
    # decisions are a codeword; with maxiter 1 the frames at 0 dB leave through the other exit
    fast = awgn_llr(Hi, M, 12.0 + max(0.0, 10.0 * np.log10(0.5 * nh / max(nh - rh, 1))), 2730 + no, FRAMES // 2, burn_codeword=False)
    out = {"awgn 0 dB": awgn_llr(Hi, M, 0.0, 2710 + no, FRAMES, burn_codeword=False),
           "awgn 2 dB": awgn_llr(Hi, M, 2.0, 2720 + no, FRAMES, burn_codeword=False),
           "adversarial, +-0.0 on resident columns": np.ascontiguousarray(adv),
           "both exits": np.concatenate([fast, 3.0 * _signs(2740 + no, (FRAMES // 2, N))])}
    for v in out.values():
        v.setflags(write=False)
    return out


def test_the_inputs_hold_what_they_are_meant_to_exercise():
    for case in CODES:
        H = CODES[case]()
        for name, llr in _inputs(case).items():
            assert llr.shape[1] == H.shape[1] * M and 1 <= llr.shape[0] <= 256 and np.isfinite(llr).all(), (case, name)
        adv = _inputs(case)["adversarial, +-0.0 on resident columns"]
        for k in nonlocal_columns(H)[:resident_columns(H, False)]:
            assert np.signbit(adv[0, k * M:(k + 1) * M]).all() and (adv[0, k * M:(k + 1) * M] == 0).all(), (case, k)


def _without_soft(dec):
    return dec.lib.ldpc_hip_last_launch_without_soft(dec.h)


def _expect_equal_both_ways(dec, oracle, llr, maxiter, what, torch):
    """without soft_out, with it, and without it again: the instance is chosen per launch"""
    d_ref, it_ref, _ = oracle.decode(MS_DEC, llr, maxiter, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, llr, maxiter, 1)
    x = torch.from_numpy(np.array(llr)).cuda()   # (a copy: the shared inputs are read-only)
    for want_soft in (False, True, False):
        hard, iters, soft = dec.decode(x, maxiter, want_soft=want_soft)
        torch.cuda.synchronize()
        assert _without_soft(dec) == (0 if want_soft else 1), (what, want_soft)
        assert np.array_equal(iters.cpu().numpy(), it_ref), (what, want_soft, iters.cpu().numpy(), it_ref)
        assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)), (what, want_soft)
        if want_soft:
            assert_bits_equal(soft.cpu().numpy(), s_ref, "soft values, " + what)
    return it_ref


@gpu
@pytest.mark.parametrize("case", list(CODES))
def test_ms_m64_with_resident_channel_values_equals_the_oracle_with_and_without_soft_values(case):
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = CODES[case]()
    oracle = Oracle(H, M)
    seen = []
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        if case == "shipped_16x32":
            assert dec.kernel_name == AOT_NAME, dec.kernel_name
        else:
            assert "ms_m64_body" in dec.kernel_name and "hiprtc" in dec.kernel_name, dec.kernel_name
        for name, llr in _inputs(case).items():
            for maxiter in (1, 2, 3, 50):
                it = _expect_equal_both_ways(dec, oracle, llr, maxiter, f"{case}, {name}, maxiter {maxiter}", torch)
                seen.append(it)
                print(case, name, "maxiter", maxiter, "iterations", it.tolist())
        assert dec.last_launch() == dec.kernel_name
    seen = np.concatenate(seen)
    assert (seen > 0).any() and (seen < 0).any(), "both exits of the iteration loop"


@gpu
def test_a_persistent_wave_of_the_shipped_instances_refills_its_slots_for_the_next_frame():
    """4096 frames, twice the 2048 resident waves of an MI355X, frames that converge at once alternating with frames that never do:
    a wave's second frame finds the resident channel values, and the bit word, of a frame that stopped at another iteration."""
    import torch

    import ldpc_lib_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    H = _shipped()
    both = _inputs("shipped_16x32")["both exits"]
    oracle = Oracle(H, M)
    d_ref, it_ref, _ = oracle.decode(MS_DEC, both, 50, 0)
    s_ref, _, _ = oracle.decode(MS_DEC, both, 50, 1)
    assert ((it_ref[:FRAMES // 2] >= 1) & (it_ref[:FRAMES // 2] <= 2)).all() and (it_ref[FRAMES // 2:] == -50).all(), it_ref
    idx = np.random.RandomState(2799).randint(0, FRAMES // 2, size=4096)
    idx[1::2] += FRAMES // 2   # even places: a frame that converges at once, odd places: one that never does
    x = torch.from_numpy(both[idx]).cuda()
    with ldpc_lib_amd.LdpcHip(MS_DEC, H, M) as dec:
        assert dec.kernel_name == AOT_NAME, dec.kernel_name
        for want_soft in (False, True):
            hard, iters, soft = dec.decode(x, 50, want_soft=want_soft)
            torch.cuda.synchronize()
            assert dec.last_launch() == AOT_NAME and _without_soft(dec) == (0 if want_soft else 1), (dec.last_launch(), want_soft)
            bad = np.flatnonzero(iters.cpu().numpy() != it_ref[idx])
            assert not bad.size, (want_soft, [(int(f), int(idx[f])) for f in bad[:8]])
            assert np.array_equal(hard.cpu().numpy().view(np.uint32), pack_bits(d_ref)[idx]), want_soft
            if want_soft:
                assert_bits_equal(soft.cpu().numpy(), s_ref[idx], "soft values")
