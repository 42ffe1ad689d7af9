"""CPU model of the LDS image and read addressing of gemm_conv_dw_tr_kernel
(caffeonspark_amd/ops/csrc/gemm.hip): DMA staging of the K-major dW operands
and the ds_read_b64_tr_b16 fragment reads.

One K tile is three [32 k][128 col] bf16 sub-images of 256-byte rows: A (dy,
128 m) and the two 128-column halves of the 256-wide col tile.  dw_tr_off
below mirrors dw_tr_off in gemm.hip — change both together.
"""

import itertools

import pytest

ROWS, CHUNKS = 32, 16          # k-rows per tile, 16-byte chunks per row
SUB = ROWS * 256               # bytes of one sub-image
WAVES, LANES = 8, 64


def dw_tr_off(row, ch):
    """Mirror of dw_tr_off in gemm.hip: byte offset of 16-byte chunk ch of
    k-row `row` inside a sub-image."""
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)))


def staged_source(wave, lane):
    """(k-row, source chunk) the kernel's staging lane fetches; its DMA lands
    at byte 1024*wave + 16*lane of the sub-image (DMA writes LDS linearly)."""
    srow = wave * 4 + (lane >> 4)
    sch = (dw_tr_off(srow, lane & 15) >> 4) & 15
    return srow, sch


def build_image():
    """byte offset -> (k-row, column) of the 16-bit element stored there."""
    img = {}
    for wave, lane in itertools.product(range(WAVES), range(LANES)):
        row, ch = staged_source(wave, lane)
        pos = 1024 * wave + 16 * lane
        for e in range(8):
            img[pos + 2 * e] = (row, 8 * ch + e)
    return img


def frag_addr(operand, wm, wn, f, h, lane):
    """The kernel's byte address (within the 3-sub-image stage) of the
    transposed read h of fragment f, exactly as it computes it: fragment
    0's address XOR (f << 5)."""
    fq, fp, fg = (lane >> 2) & 3, lane & 3, lane >> 4
    row = 8 * fg + 4 * h + fq
    if operand == "A":
        base = dw_tr_off(row, wm * 8 + (fp >> 1)) + 8 * (fp & 1)
    else:
        base = ((1 + (wn >> 1)) * SUB +
                dw_tr_off(row, (wn & 1) * 8 + (fp >> 1)) + 8 * (fp & 1))
    return base ^ (f << 5)


def frag_origin(operand, wm, wn, f):
    """(sub-image index, first column within it) of the fragment."""
    if operand == "A":
        return 0, wm * 64 + f * 16
    return 1 + (wn >> 1), (wn & 1) * 64 + f * 16


POSITIONS = [("A", wm, 0) for wm in range(2)] + \
            [("B", 0, wn) for wn in range(4)]


def test_staging_is_a_bijection():
    # the A image and each B half use the same lane -> chunk map
    seen_src, seen_pos = set(), set()
    for wave, lane in itertools.product(range(WAVES), range(LANES)):
        row, ch = staged_source(wave, lane)
        pos = 1024 * wave + 16 * lane
        assert 0 <= row < ROWS and 0 <= ch < CHUNKS
        # staging and reading go through the same off function
        assert pos == dw_tr_off(row, ch)
        seen_src.add((row, ch))
        seen_pos.add(pos)
    assert len(seen_src) == ROWS * CHUNKS
    assert seen_pos == set(range(0, SUB, 16))
    # the B image: column n of the 256-wide tile lives in half n >> 7
    cols = set()
    for half, (row, ch) in itertools.product(range(2), sorted(seen_src)):
        cols.update((row, half * 128 + 8 * ch + e) for e in range(8))
    assert len(cols) == ROWS * 256


@pytest.mark.parametrize("operand,wm,wn", POSITIONS)
def test_fragment_contents(operand, wm, wn):
    img = build_image()
    for f, h in itertools.product(range(4), range(2)):
        sub, col0 = frag_origin(operand, wm, wn, f)
        addr = [frag_addr(operand, wm, wn, f, h, lane)
                for lane in range(LANES)]
        for a in addr:
            assert a % 8 == 0 and sub * SUB <= a < (sub + 1) * SUB
        for g, i in itertools.product(range(4), range(16)):
            # lane 4q+p of the group supplies row q, columns 4p..4p+3;
            # lane i receives column i, row q in element q
            for q in range(4):
                src = addr[16 * g + 4 * q + (i >> 2)] - sub * SUB
                got = img[src + 2 * (i & 3)]
                assert got == (8 * g + 4 * h + q, col0 + i), \
                    (operand, wm, wn, f, h, g, i, q, got)


@pytest.mark.parametrize("operand,wm,wn", POSITIONS)
def test_bank_conflicts_at_most_two_way(operand, wm, wn):
    worst = 0
    for f, h in itertools.product(range(4), range(2)):
        for half in range(2):
            banks = {}
            for lane in range(32 * half, 32 * half + 32):
                a = frag_addr(operand, wm, wn, f, h, lane)
                for dw in (a // 4, a // 4 + 1):     # 8 bytes = 2 banks
                    banks.setdefault(dw % 64, set()).add(dw)
            worst = max(worst, max(len(v) for v in banks.values()))
    assert worst <= 2, worst


def test_xor_shortcut_matches_off():
    """fragment f's address is fragment 0's ^ (f << 5): the same as going
    through dw_tr_off with chunk c0 + 2f + p/2."""
    for (operand, wm, wn), f, h, lane in itertools.product(
            POSITIONS, range(4), range(2), range(LANES)):
        fq, fp, fg = (lane >> 2) & 3, lane & 3, lane >> 4
        row = 8 * fg + 4 * h + fq
        sub, col0 = frag_origin(operand, wm, wn, f)
        want = sub * SUB + dw_tr_off(row, col0 // 8 + (fp >> 1)) + 8 * (fp & 1)
        assert frag_addr(operand, wm, wn, f, h, lane) == want
