"""The index contract of csrc/conv_wino4.hip's segment form, restated on numpy integers (no GPU, no library): the planner
(rectangular blocks vs runs of R (image, tile row) units, the same cost on both sides), the per-item segment table, the raw-block
gather (load slot -> plane entry and input pixel), the transform's per-slot plane base and the tile table of the epilogue.
tests/test_wino4_segments_layout.py checks the maps against each other and the planner against the library's own
(w2l_wino4_block_plan)."""
import numpy as np

BT = 32                 # tile slots per work item
RAW_PIX = 768           # pixels of a raw block (3 load slots x 512 threads / 2 channel quads)
PS = 202                # cells per raw plane; entry = q * 4 * PS + (x & 3) * PS + cell
RECT_CELLS = 186
S = 8                   # segments per item
RECT = [(4, 8, 1), (8, 4, 1), (4, 4, 2), (2, 8, 2), (8, 2, 1), (2, 4, 3), (4, 2, 3), (3, 3, 3),
        (2, 2, 6), (2, 3, 4), (3, 2, 4), (1, 4, 6), (4, 1, 5), (1, 2, 10), (2, 1, 9), (1, 1, 15)]
GROUPS = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31))


def cdiv(a, b):
    return -(-a // b)


def rect_cost(N, TH, TW):
    best = None
    for bh, bw, ni in RECT:
        RH, RW = 4 * bh + 2, 4 * bw + 2
        if bh * bw * ni > BT or ni * RH * RW > RAW_PIX or ni * RH * (bw + 1) > RECT_CELLS:
            continue
        items = cdiv(TH, bh) * cdiv(TW, bw) * cdiv(N, ni)
        cost = items * (1.0 + 0.05 * (RH * RW) / (16.0 * bh * bw))
        if best is None or cost < best[0]:
            best = (cost, items, (bh, bw, ni))
    return best


def seg_count(off, R, TH):
    return (off + R - 1) // TH + 1


def seg_worst(R, TH, nblk):
    return max(seg_count((b * R) % TH, R, TH) for b in range(min(nblk, TH)))


def conflicts(R, TH, TW, nblk, pitch, pad):
    cost = 0
    for b in range(min(nblk, TH)):
        off = (b * R) % TH
        for g in range(4):
            cnt = [0] * 16
            for k in GROUPS[g & 1]:
                lane = k + 32 * (g >> 1)
                tl, q = lane >> 1, lane & 1
                r, c = divmod(tl, TW)
                if r >= R:
                    r = c = 0
                j = (off + r) // TH
                cnt[(q * 4 * PS + (4 * r + 2 * j) * pitch + j * pad + c) & 15] += 1
            cost += sum((n - 1) * 64 * n for n in cnt if n > 1)
    return cost


def pick_seg(N, TH, TW):
    """-> (R, pitch, pad, blocks, cost) or None: the most rows per block under the slot, raw-pixel and plane-cell limits"""
    units, RW = N * TH, 4 * TW + 2
    for R in range(min(BT // TW, units), 0, -1):
        nblk = cdiv(units, R)
        ns = seg_worst(R, TH, nblk)
        rows = 4 * R + 2 * ns
        if ns > S or rows * RW > RAW_PIX or rows * (TW + 1) > PS:
            continue
        cost = nblk * (1.0 + 0.05 * (rows * RW) / (16.0 * R * TW))
        best = None
        for p in range(TW + 1, TW + 5):
            for pad in range(8):
                if rows * p + (ns - 1) * pad > PS:
                    break
                c = conflicts(R, TH, TW, nblk, p, pad) + (p - TW - 1) + pad
                if best is None or c < best[0]:
                    best = (c, p, pad)
        return R, best[1], best[2], nblk, cost
    return None


def plan(N, H, W):
    """what w2l_wino4_block_plan returns in out[0:7]"""
    TH, TW = cdiv(H, 4), cdiv(W, 4)
    rc, ritems, rb = rect_cost(N, TH, TW)
    sg = pick_seg(N, TH, TW)
    if sg is not None and sg[4] < rc:
        return (1, sg[3], sg[0], TW, 0, sg[1], sg[2])
    return (0, ritems) + rb


def segment_table(blk, R, N, TH, TW, pitch, pad):
    """rows {image, first tile row, tile rows, first raw row, first plane cell, first tile slot} of one item"""
    u0 = blk * R
    u1 = min(u0 + R, N * TH)
    nfirst = u0 // TH
    tab = np.zeros((S, 6), dtype=np.int64)
    for t in range(S):
        n = nfirst + t
        ua, ub = max(u0, n * TH), min(u1, (n + 1) * TH)
        row0 = ua - u0
        tab[t] = (n, ua - n * TH, max(ub - ua, 0), 4 * row0 + 2 * t, (4 * row0 + 2 * t) * pitch + t * pad, row0 * TW)
    return tab


def gather(tab, H, W, TW, pitch):
    """load slot e < 1536 -> (plane entry or -1, (image, y, x) or None): the raw-block gather of one K-step"""
    RW = 4 * TW + 2
    out = []
    for e in range(2 * RAW_PIX):
        q, pix = (e >> 3) & 1, (e >> 4) * 8 + (e & 7)
        p2 = int((np.float32(pix) + np.float32(0.5)) * np.float32(1.0 / RW))
        rxx = pix - p2 * RW
        j = 0
        for s in range(1, S):
            if tab[s, 2] > 0 and p2 >= tab[s, 3]:
                j = s
        n, ty0, nr, rr0, cell0, _ = tab[j]
        ry = p2 - rr0
        if ry >= 4 * nr + 2:
            out.append((-1, None))
            continue
        entry = q * 4 * PS + (rxx & 3) * PS + cell0 + ry * pitch + (rxx >> 2)
        iy, ix = 4 * ty0 - 1 + ry, rxx - 1
        out.append((int(entry), (int(n), int(iy), int(ix)) if 0 <= iy < H and 0 <= ix < W else None))
    return out


def slots(blk, R, N, H, W, TH, TW, pitch, pad):
    """tile slot -> (image, ty, tx) or None, and the q = 0 plane cell of the slot's patch origin (unused slots: slot 0's)"""
    u0 = blk * R
    u1 = min(u0 + R, N * TH)
    nfirst = u0 // TH
    tiles, bases = [], []
    for tl in range(BT):
        r, txl = divmod(tl, TW)
        tiles.append(((u0 + r) // TH, (u0 + r) % TH, txl) if u0 + r < u1 else None)
        if u0 + r >= u1:
            r = txl = 0
        j = (u0 + r) // TH - nfirst
        bases.append((4 * r + 2 * j) * pitch + j * pad + txl)
    return tiles, bases
