"""CPU model of the staged n_fft-512 kernel's power-tile layout (modulation_mfcc_amd/csrc/mm_s16.h, mm_logmel16s.hip.inc):
the 16x16 exchange written with ds_write_addtid_b32 into each wave's own power rows, its b128 reads, and phase B's
lane-per-frame b128 reads at the s16 row pitch.  Bank groups are the MI355X LDS lane groups of each instruction."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "modulation_mfcc_amd", "csrc")

# ds_read_b128: four groups of sixteen lanes, one LDS cycle each when their 64 dwords fall on 64 distinct banks
B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]
# ds_write_b32 / ds_write_addtid_b32: two groups of 32 lanes, bank = dword address mod 32
B32_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def _addtid_pitch():
    """The row pitch of the instantiations that write the exchange with ds_write_addtid_b32 (MM_S16_XA_PITCH: the XA instantiations)."""
    src = open(os.path.join(CSRC, "mm_s16.h")).read()
    m = re.search(r"#define MM_S16_XA_PITCH (\d+)", src)
    assert m
    return int(m.group(1))


PITCH = _addtid_pitch()


def xb(k1):
    """mm_s16_xb(k1): float offset of register k1's 64-lane block in the wave's exchange area."""
    m = k1 if k1 < 4 else (k1 - 8 if k1 >= 12 else k1 - 4)
    j = 2 * m + (1 if 4 <= k1 < 12 else 0)
    return 64 * j + 4 * ((m & 3) + 8 * (m >> 2))


def test_xb_matches_the_header():
    """The header pins mm_s16_xb's sixteen values with a static_assert: the model must give the same ones."""
    src = open(os.path.join(CSRC, "mm_s16.h")).read()
    pinned = {int(k): int(v) for k, v in re.findall(r"mm_s16_xb\((\d+)\) == (\d+)", src)}
    assert sorted(pinned) == list(range(16))
    assert all(pinned[k] == xb(k) for k in range(16)), pinned


def ex_write(k1, lane):
    """s16_ex_store: ds_write_addtid_b32 of register k1, lane l -> area + mm_s16_xb(k1) + l."""
    return xb(k1) + lane


def ex_read(i, lane):
    """Exchange read i (rq0 .. rq3) of lane (row, q): block q, row `row`, chunk i -> registers 4 i .. 4 i + 3."""
    row, q = lane >> 4, lane & 15
    return xb(q) + 16 * row + 4 * i


def _b128_conflict_free(addr_of_lane):
    for g in B128_GROUPS:
        banks = [(addr_of_lane(l) + d) % 64 for l in g for d in range(4)]
        if len(set(banks)) != 64:
            return False
    return True


def test_pitch_holds_the_exchange_and_the_pad_bins():
    area = max(xb(k1) + 64 for k1 in range(16))
    assert area == 1068
    assert 4 * PITCH >= area                   # the exchange stays inside the wave's own four power rows
    assert PITCH >= 260 and PITCH % 4 == 0     # bins 0 .. 256 + three pad bins, 16-byte aligned rows


def test_exchange_blocks_are_disjoint_and_16_byte_aligned():
    cells = [ex_write(k1, l) for k1 in range(16) for l in range(64)]
    assert len(set(cells)) == 16 * 64
    assert all(xb(k1) % 4 == 0 for k1 in range(16))


def test_exchange_round_trip():
    """Lane (row, q) reads back exactly column n2 = 0..15 of register k1 = q of its own frame."""
    where = {}
    for k1 in range(16):
        for l in range(64):
            where[ex_write(k1, l)] = (k1, l)
    for l in range(64):
        row, q = l >> 4, l & 15
        for i in range(4):
            a = ex_read(i, l)
            assert a % 4 == 0
            for d in range(4):
                k1, src = where[a + d]
                assert k1 == q and src >> 4 == row and (src & 15) == 4 * i + d


def test_exchange_reads_conflict_free():
    for i in range(4):
        assert _b128_conflict_free(lambda l: ex_read(i, l)), i


def test_exchange_writes_conflict_free():
    for k1 in range(16):
        for g in B32_GROUPS:
            assert len({ex_write(k1, l) % 32 for l in g}) == 32


def test_phase_b_reads_conflict_free():
    # lane = frame, all lanes read the same group of four bins k4 .. k4 + 3 of their own row
    for k4 in range(0, 260, 4):
        assert _b128_conflict_free(lambda l: l * PITCH + k4), k4


def test_power_rows_inside_p_and_pads_behind_bin_256():
    # every (frame, bin) cell of phase A's stores and phase B's reads (bins 0 .. 259) is distinct and inside P
    cells = {f * PITCH + k for f in range(64) for k in range(260)}
    assert len(cells) == 64 * 260
    assert max(cells) < 64 * PITCH
    # the exchange areas of the sixteen waves stay inside P and apart
    ex = [4 * w * PITCH + ex_write(k1, l) for w in range(16) for k1 in range(16) for l in range(64)]
    assert len(set(ex)) == len(ex) and max(ex) < 64 * PITCH
