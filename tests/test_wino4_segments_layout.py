"""The index contract of conv_wino4.hip's segment form without a GPU (tools/wino4_seg_emulate.py restates the planner, the
per-item segment table, the raw-block gather and the slot -> patch maps): over every N <= 9 and TH, TW <= 8 each tile has exactly
one owner, an item stays inside the raw buffer and the planes, every slot's 6 x 6 patch reads the entries its own image's pixels
were staged at, and the rows per block are the ones the library picks."""
import ctypes
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import wino4_seg_emulate as em  # noqa: E402

SHAPES = [(N, TH, TW) for N in range(1, 10) for TH in range(1, 9) for TW in range(1, 9)]


def test_rows_per_block_for_the_generator_layers():
    """12x12 packs 10 tile rows (30 of 32 slots, 39 blocks for 128 frames: 234 items at 384 couts, one round of 256 CUs), 24x24 five
    rows of six (154 blocks against 172 rectangles); 96x96 and 48x48 keep their full 4x8x1 and 4x4x2 rectangles"""
    assert em.plan(128, 12, 12)[:4] == (1, 39, 10, 3)
    assert em.plan(128, 24, 24)[:4] == (1, 154, 5, 6)
    assert em.plan(128, 96, 96)[:5] == (0, 2304, 4, 8, 1)
    assert em.plan(128, 48, 48)[:5] == (0, 576, 4, 4, 2)
    # a uniform stride per segment would not fit (4 x 14 x 14 pixels): the worst split of ten rows is 1+3+3+3 = 48 raw rows
    assert em.seg_worst(10, 3, 39) == 4 and (4 * 10 + 2 * 4) * 14 <= em.RAW_PIX < 4 * 14 * 14
    assert em.seg_worst(5, 6, 154) == 2 and (4 * 5 + 2 * 2) * 26 <= em.RAW_PIX


def test_planner_is_the_librarys():
    from wav2lip_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 8)()
    for N, TH, TW in SHAPES + [(128, 3, 3), (128, 6, 6), (128, 24, 24), (128, 12, 12), (128, 2, 2), (64, 3, 3), (256, 6, 6)]:
        for H, W in ((4 * TH, 4 * TW), (4 * TH - 1, 4 * TW - 3)):
            assert lib.w2l_wino4_block_plan(N, H, W, out) == 0
            want = em.plan(N, H, W)
            got = tuple(out)[:7]
            assert got[:5] == want[:5] and out[7] == em.PS, (N, H, W, got, want)
            if want[0]:
                assert got[5:7] == want[5:7], (N, H, W, got, want)
    assert lib.w2l_wino4_block_plan(0, 4, 4, out) != 0


@pytest.mark.parametrize("N", range(1, 10))
def test_every_tile_has_one_owner_and_every_patch_reads_its_own_pixels(N):
    for TH in range(1, 9):
        for TW in range(1, 9):
            sg = em.pick_seg(N, TH, TW)
            if sg is None:
                continue
            R, pitch, pad, nblk, _ = sg
            H, W = 4 * TH - (TH & 1), 4 * TW - (N % 3)         # ragged last tile row / column on some shapes
            assert R * TW <= em.BT and nblk == em.cdiv(N * TH, R)
            owners = {}
            # blocks repeat with the period of their start row inside an image: check each start once, plus the first and last
            seen = set()
            for blk in range(nblk):
                tiles, bases = em.slots(blk, R, N, H, W, TH, TW, pitch, pad)
                for tl, tile in enumerate(tiles):
                    if tile is not None:
                        assert tile not in owners and tile[0] < N and tile[1] < TH and tile[2] < TW, (N, TH, TW, blk, tl)
                        owners[tile] = (blk, tl)
                key = ((blk * R) % TH, min(R, N * TH - blk * R))
                if key in seen:
                    continue
                seen.add(key)
                tab = em.segment_table(blk, R, N, TH, TW, pitch, pad)
                assert tab[:, 2].sum() == min(R, N * TH - blk * R)
                staged = {}
                npix = 0
                for entry, pixel in em.gather(tab, H, W, TW, pitch):
                    if entry < 0:
                        continue
                    q, rest = divmod(entry, 4 * em.PS)
                    assert q < 2 and rest % em.PS < em.PS and entry not in staged, (N, TH, TW, blk, entry)
                    staged[entry] = pixel
                    npix += q == 0
                rows = int((4 * tab[:, 2] + 2 * (tab[:, 2] > 0)).sum())
                assert npix == rows * (4 * TW + 2) <= em.RAW_PIX
                cells = {e % em.PS for e in staged}
                assert max(cells) < em.PS and max(e // em.PS for e in staged) < 8
                for tl, tile in enumerate(tiles):
                    for a in range(6):
                        for c in range(6):
                            entry = (c & 3) * em.PS + bases[tl] + a * pitch + (c >> 2)
                            assert entry in staged, (N, TH, TW, blk, tl, a, c)       # unused slots too: a read inside the block
                            if tile is None:
                                continue
                            n, ty, tx = tile
                            iy, ix = 4 * ty - 1 + a, 4 * tx - 1 + c
                            want = (n, iy, ix) if 0 <= iy < H and 0 <= ix < W else None
                            assert staged[entry] == want and staged[entry + 4 * em.PS] == want, (N, TH, TW, blk, tl, a, c)
            assert len(owners) == N * TH * TW
