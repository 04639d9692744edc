"""CPU model of the transposed read-back of csrc/rank_rows.hip (``RRRead``).

After a 2-byte exchange scatter every lane fetches the values that landed in its own slots: slot ``wave * 64 * ITEMS + 64 * s + L`` of
the exchange buffer for step ``s`` of lane ``L``.  ``RRRead`` takes four steps per LDS instruction with gfx950's
``ds_read_b64_tr_b16``: per group of 16 lanes the instruction reads a block of 4 rows x 16 columns of 16-bit elements; lane ``4q + p``
of the group supplies the address of row ``q``, columns ``4p .. 4p + 3``; lane ``i`` of the group receives column ``i`` of the four
rows, row ``q`` in element ``q``.  The "rows" are four consecutive steps of the wave's slice (128 bytes apart), the "columns" the
group's 16 lane positions.  A misaligned address returns the aligned address's data and raises nothing, and a read behind wave 7's
slice would leave the LDS allocation, so this file holds the address recipe to the instruction's lane map for every instantiation:

    rt = xbuf + 2 * wave * (ITEMS * 64) + 128 * q + 32 * g + 8 * p,      read k at rt + 512 * k,   k < ITEMS // 4

and the four ``v_perm_b32`` selectors that merge either half of a returned dword into the high or the low half of a live register.
"""
import re
import os

import numpy as np
import pytest

ITEMS_TABLE = (2, 8, 12, 20, 30, 40, 46, 52, 58, 64, 72, 80, 88, 98, 104)
WAVES, WAVE = 8, 64
XBUF = 0x4A80        # a byte address of the exchange buffer in LDS: any multiple of 16 (rr_raw is 16-byte aligned, every carve is too)
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "semantic-embeddings_amd", "csrc", "rank_rows.hip")


def lane_address(items, wave, lane, k):
    """Part 1 of the recipe: the byte address lane ``lane`` of wave ``wave`` supplies to transposed read ``k``."""
    g, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
    return XBUF + 2 * wave * (items * WAVE) + 128 * q + 32 * g + 8 * p + 512 * k


def tr_read(lds, addr):
    """ds_read_b64_tr_b16 on one wave.  lds: the LDS as uint16 elements (index = byte address / 2); addr[64]: every lane's byte
    address.  -> [64, 4] uint16: the four elements lane L receives (element 0 = low half of the first dword)."""
    out = np.zeros((WAVE, 4), dtype=np.uint16)
    for grp in range(4):
        block = np.zeros((4, 16), dtype=np.uint16)                 # 4 rows x 16 columns
        for q in range(4):
            for p in range(4):
                a = int(addr[16 * grp + 4 * q + p])
                a -= a % 8                                         # the hardware drops the low address bits: wrong data, no fault
                block[q, 4 * p:4 * p + 4] = lds[a // 2:a // 2 + 4]
        for i in range(16):
            out[16 * grp + i] = block[:, i]                        # column i, row q in element q
    return out


def perm(s0, s1, sel):
    """v_perm_b32 D, S0, S1, sel: byte i of D is byte sel[i] of the 8 bytes {S0 (bytes 4-7), S1 (bytes 0-3)}."""
    src = (int(s0) << 32) | int(s1)
    d = 0
    for i in range(4):
        b = (sel >> (8 * i)) & 0xFF
        assert b < 8
        d |= ((src >> (8 * b)) & 0xFF) << (8 * i)
    return d


def kernel_selectors():
    """The four selectors as rank_rows.hip states them: {(HI, half): selector}."""
    text = open(SRC).read()
    lo = re.search(r"SEL_LO16 = HI \? (0x[0-9A-Fa-f]+)u : (0x[0-9A-Fa-f]+)u", text)
    hi = re.search(r"SEL_HI16 = HI \? (0x[0-9A-Fa-f]+)u : (0x[0-9A-Fa-f]+)u", text)
    assert lo and hi, "RRRead's selectors not found in rank_rows.hip"
    return {(True, 0): int(lo.group(1), 16), (False, 0): int(lo.group(2), 16), (True, 1): int(hi.group(1), 16), (False, 1): int(hi.group(2), 16)}


@pytest.mark.parametrize("items", ITEMS_TABLE)
def test_every_lane_receives_its_own_slots(items):
    slots = WAVES * WAVE * items
    lds = np.full(XBUF // 2 + slots + 64, 0xDEAD, dtype=np.uint16)
    vals = ((np.arange(slots, dtype=np.int64) * 40503 + 12345) % 65521).astype(np.uint16)        # distinct: 40503 is prime to 65521 > slots
    assert len(np.unique(vals)) == slots
    lds[XBUF // 2:XBUF // 2 + slots] = vals
    nt = items // 4
    covered = np.zeros((WAVES, items), dtype=bool)
    for wave in range(WAVES):
        for k in range(nt):
            addr = np.array([lane_address(items, wave, lane, k) for lane in range(WAVE)])
            assert (addr % 8 == 0).all()
            assert (addr >= XBUF).all() and (addr + 8 <= XBUF + 2 * 512 * items).all()
            # inside the wave's OWN slice, too: the other waves' slices are theirs to read
            assert (addr >= XBUF + 128 * items * wave).all() and (addr + 8 <= XBUF + 128 * items * (wave + 1)).all()
            got = tr_read(lds, addr)
            for e in range(4):
                s = 4 * k + e
                want = vals[wave * WAVE * items + WAVE * s + np.arange(WAVE)]
                assert np.array_equal(got[:, e], want), (items, wave, k, e)
                covered[wave, s] = True
    # the tail: exactly the steps the transposed reads do not cover keep the 16-bit read
    tail = [s for s in range(items) if s >= 4 * nt]
    assert len(tail) == items % 4 == (2 if items in (2, 30, 46, 58, 98) else 0)
    for wave in range(WAVES):
        assert [s for s in range(items) if not covered[wave, s]] == tail


def test_model_returns_wrong_data_for_a_misaligned_address():
    """The model is not blind to what it guards against: the same recipe on a buffer 4 bytes off its alignment fails."""
    lds = np.arange(4096, dtype=np.uint16)
    addr = np.array([lane_address(8, 0, lane, 0) - XBUF + 4 for lane in range(WAVE)])
    got = tr_read(lds, addr)
    assert not np.array_equal(got[:, 0], lds[2 + np.arange(WAVE)])


def test_code_states_the_recipe():
    text = open(SRC).read()
    assert "return 128u * ((lane >> 2) & 3u) + 32u * (lane >> 4) + 8u * (lane & 3u);" in text
    assert "rt = xb + 2u * (uint32_t)(wave * (ITEMS * WAVE)) + rr_tr_lane_off((uint32_t)lane);" in text
    assert "lds_ld16x4_tr<I * 4 * WAVE * 2>" in text                       # read k at 512 k
    assert "lds_ld16<(3 * NT + I) * WAVE * 2>(u[I - NT], rb)" in text      # the tail: step 4 NT + (I - NT) at rb + 128 step


def test_perm_selectors_on_packed_pairs():
    sel = kernel_selectors()
    assert sel == {(True, 0): 0x05040100, (True, 1): 0x07060100, (False, 0): 0x03020504, (False, 1): 0x03020706}
    rng = np.random.default_rng(0)
    for _ in range(64):
        t, a = (int(x) for x in rng.integers(0, 1 << 32, size=2, dtype=np.uint64))
        halves = (t & 0xFFFF, t >> 16)                                     # elements 2j and 2j + 1 of a read, as packed in dword j
        for half in (0, 1):
            assert perm(t, a, sel[(True, half)]) == (halves[half] << 16) | (a & 0xFFFF)
            assert perm(t, a, sel[(False, half)]) == (a & 0xFFFF0000) | halves[half]
