"""w2l_frame_hist_rows and w2l_scene_cuts (csrc/scene.hip; scene-cut detection) against the model of
tests/_scene_cases.py: exact equality everywhere, poisoned bytes around every frame, guard rows around every output."""
import ctypes

import numpy as np
import pytest
import torch

import _scene_cases as sc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 2, 0x5A5A5A5A            # guard rows of 96 words on either side of the signature rows
OFFSETS = (0, 1, 2, 3, 5, 15, 16, 17)      # byte offsets of a frame from a 256-byte aligned base
POISON = 64                                # poisoned bytes before and after every frame: more than a 48-byte unit


# ---------------------------------------------------------------- w2l_frame_hist_rows
class Carved:
    """frames of one shape carved out of ONE uint8 device buffer: frame k starts `offset` bytes after a 256-byte aligned base, and
    the POISON bytes before and after it hold a value from a bin the frame does not use (any value where it uses all of them: a
    counted over-read then still breaks the channel sums)"""

    def __init__(self, frames, offset, dev):
        self.frames = frames
        nbytes = frames[0].size
        slot = (POISON + offset + nbytes + POISON + 255) // 256 * 256 + 256
        host = np.zeros(slot * len(frames) + 256, np.uint8)
        starts = []
        for k, f in enumerate(frames):
            base = slot * k + 256                  # the buffer itself is 256-byte aligned (checked below)
            poison = sc.unused_byte(f)
            host[base - POISON:base + offset + nbytes + POISON] = 0x55 if poison is None else poison
            host[base + offset:base + offset + nbytes] = f.reshape(-1)
            starts.append(base + offset)
        self.buffer = torch.from_numpy(host).to(dev)
        assert self.buffer.data_ptr() % 256 == 0
        self.addresses = [self.buffer.data_ptr() + s for s in starts]

    def table(self, picks):
        return torch.tensor([self.addresses[k] for k in picks], dtype=torch.int64, device=self.buffer.device)


def device_signatures(table, B, H, W, dev):
    """the product's wrapper on an address table, the B rows between guard rows -> numpy int64 [B,96]"""
    from wav2lip_amd.face_detection.scene import frame_signatures
    whole = torch.full((B + 2 * GUARD, sc.WORDS), SENTINEL, dtype=torch.int32, device=dev)
    frame_signatures(table, whole, GUARD, rows=(B, H, W))
    h = whole.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + B:] == SENTINEL).all(), "guard rows were written"
    return h[GUARD:GUARD + B].astype(np.int64)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (5, 7), (16, 16), (17, 23), (96, 96), (123, 211)])
def test_signatures_equal_the_model_at_every_offset_and_content(cuda, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    frames = [sc.content(kind, H, W, rng) for kind in sc.CONTENTS]
    want = sc.signatures(frames)
    assert (want.reshape(len(frames), 3, sc.BINS).sum(axis=2) == H * W).all()
    for offset in OFFSETS:
        carved = Carved(frames, offset, cuda)
        # B = 6 (every content), 1, 2 with a repeated address (the padded tail of a group), 5 with one
        for picks in (list(range(len(frames))), [4], [1, 1], [0, 2, 3, 5, 5]):
            got = device_signatures(carved.table(picks), len(picks), H, W, cuda)
            assert (got == want[picks]).all(), (offset, picks, np.argwhere(got != want[picks])[:4].tolist())
    again = device_signatures(carved.table(list(range(len(frames)))), len(frames), H, W, cuda)
    assert (again == want).all()                                                   # a second launch: identical words


@pytest.mark.parametrize("H,W,offset", [(480, 640, 0), (481, 643, 5)])
def test_a_frame_that_spans_many_workgroups_and_ends_ragged(cuda, H, W, offset):
    rng = np.random.default_rng(W)
    frames = [sc.content("random", H, W, rng), sc.content("channels", H, W, rng)]
    want = sc.signatures(frames)
    carved = Carved(frames, offset, cuda)
    for k in range(2):                                                             # one frame each
        got = device_signatures(carved.table([k]), 1, H, W, cuda)
        assert (got == want[[k]]).all(), (k, np.argwhere(got != want[[k]])[:4].tolist())
    assert (device_signatures(carved.table([0]), 1, H, W, cuda) == want[[0]]).all()


def test_frame_signatures_takes_a_frame_tensor_and_an_arena_offset(cuda):
    from wav2lip_amd.face_detection.scene import frame_signatures
    rng = np.random.default_rng(3)
    frames = np.stack([sc.content(kind, 9, 11, rng) for kind in ("random", "ramp", "zeros")])
    sig = torch.full((7, sc.WORDS), SENTINEL, dtype=torch.int32, device=cuda)
    frame_signatures(torch.from_numpy(frames).to(cuda), sig, 2)
    h = sig.cpu().numpy()
    assert (h[2:5] == sc.signatures(frames)).all() and (h[:2] == SENTINEL).all() and (h[5:] == SENTINEL).all()
    with pytest.raises(ValueError):
        frame_signatures(torch.from_numpy(frames).to(cuda), sig, 5)               # rows [5, 8) leave the arena
    with pytest.raises(ValueError):
        frame_signatures(torch.from_numpy(frames).to(cuda), sig.long(), 0)


def test_frame_hist_rows_refuses_on_the_host(cuda):
    from wav2lip_amd._lib import current_stream, load, ptr
    lib = load()
    table = torch.zeros(4, dtype=torch.int64, device=cuda)
    sig = torch.full((4, sc.WORDS), SENTINEL, dtype=torch.int32, device=cuda)
    s = current_stream()
    for args in ((1, 4, 4, None, ptr(sig)), (1, 4, 4, ptr(table), None), (0, 4, 4, ptr(table), ptr(sig)), (-1, 4, 4, ptr(table), ptr(sig)),
                 (1, 0, 4, ptr(table), ptr(sig)), (1, 4, 0, ptr(table), ptr(sig)), (1, 1 << 15, 10923, ptr(table), ptr(sig)),
                 (1, 4, 4, ctypes.c_void_p(table.data_ptr() + 4), ptr(sig))):
        assert lib.w2l_frame_hist_rows(s, *args) != 0, args
        assert lib.w2l_last_error()
    assert 6 * (1 << 15) * 10923 >= 1 << 31 > 6 * (1 << 15) * 10922
    torch.cuda.synchronize()
    assert (sig.cpu().numpy() == SENTINEL).all()                                   # nothing was launched


# ---------------------------------------------------------------- w2l_scene_cuts
def device_cuts(segs, sig, q, dev, n_rows=None, with_dist=True):
    """w2l_scene_cuts called directly, outputs between guards -> numpy (cuts [R], dist [R] or None, status [n_seg]); rows the kernel
    did not write hold the sentinel"""
    from wav2lip_amd._lib import BOX_SEGMENT, check, current_stream, load, ptr
    table = np.zeros(len(segs), dtype=BOX_SEGMENT)
    for k, s in enumerate(segs):
        table[k] = s
    R = len(sig)
    t = torch.from_numpy(table.view(np.uint8)).to(dev)
    s_dev = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(-1, sc.WORDS)).to(dev)
    outs = [torch.full((n + 128,), SENTINEL, dtype=torch.int32, device=dev) for n in (R, R, len(segs))]
    cuts, dist, status = (o[64:o.numel() - 64] for o in outs)
    check(load().w2l_scene_cuts(current_stream(), len(segs), ptr(t), ptr(s_dev), R if n_rows is None else n_rows, q, ptr(cuts),
                                ptr(dist) if with_dist else None, ptr(status)), "scene_cuts")
    for o in outs:
        h = o.cpu().numpy()
        assert (h[:64] == SENTINEL).all() and (h[-64:] == SENTINEL).all()
    return cuts.cpu().numpy(), dist.cpu().numpy() if with_dist else None, status.cpu().numpy()


@pytest.mark.parametrize("q", [1, 255])
def test_the_bound_itself_is_no_cut_and_one_count_more_is(cuda, q):
    H = W = 16                                     # 6 H W = 1536: D * 256 == q * 1536 at D = 6 q, an even number a frame pair reaches
    d = 6 * q
    assert d * 256 == q * 6 * H * W and d + 2 <= 6 * H * W
    a, at = sc.sig_with_distance(H, W, d)
    _, over = sc.sig_with_distance(H, W, d + 2)
    one_more = at.copy()
    one_more[5] += 1                               # prescribed words: exactly one count above the bound
    sig = np.stack([a, at, a, over, a, one_more, a, a])
    cuts, dist, status = device_cuts([(0, 2, H, W), (2, 2, H, W), (4, 2, H, W), (6, 2, H, W)], sig, q, cuda)
    assert status.tolist() == [0, 0, 0, 0]
    assert cuts.tolist() == [0, 0, 0, 1, 0, 1, 0, 0]
    assert dist.tolist() == [0, d, 0, d + 2, 0, d + 1, 0, 0]
    for k in range(4):
        want, _ = sc.cut_flags(sig[2 * k:2 * k + 2], H, W, q)
        assert cuts[2 * k:2 * k + 2].tolist() == want.tolist()


def test_segments_of_every_length_in_one_launch_equal_the_model(cuda):
    H = W = 16
    rng = np.random.default_rng(11)
    base, near = sc.sig_with_distance(H, W, 6)
    _, mid = sc.sig_with_distance(H, W, 8)
    _, far = sc.sig_with_distance(H, W, 6 * H * W)
    kinds = np.stack([base, near, mid, far])
    lengths = [0, 1, 2, 63, 64, 65, 130, 0, 3]
    sig = kinds[rng.integers(0, 4, sum(lengths))]
    segs, row = [], 0
    for n in lengths:
        segs.append((row, n, H, W))
        row += n
    for q in (1, 77):
        cuts, dist, status = device_cuts(segs, sig, q, cuda)
        assert not status.any()
        fired = 0
        for r0, n, _, _ in segs:
            want_c, want_d = sc.cut_flags(sig[r0:r0 + n], H, W, q)
            assert cuts[r0:r0 + n].tolist() == want_c.tolist() and dist[r0:r0 + n].tolist() == want_d.tolist(), (q, r0, n)
            fired += int(want_c.sum())
        assert 0 < fired < len(sig) - len(lengths)                                  # not vacuous either way
        no_dist, none, _ = device_cuts(segs, sig, q, cuda, with_dist=False)        # dist may be NULL
        assert none is None and (no_dist == cuts).all()


def test_a_segments_first_row_is_never_a_cut(cuda):
    H = W = 16
    a, far = sc.sig_with_distance(H, W, 6 * H * W)
    sig = np.stack([a, a, far, far, a])            # row 2 differs from row 1 by everything, and is the second clip's first row
    cuts, dist, _ = device_cuts([(0, 2, H, W), (2, 3, H, W)], sig, 1, cuda)
    assert cuts.tolist() == [0, 0, 0, 0, 1] and dist.tolist() == [0, 0, 0, 0, 6 * H * W]
    cuts, _, _ = device_cuts([(0, 5, H, W)], sig, 1, cuda)
    assert cuts.tolist() == [0, 0, 1, 0, 1]


def test_a_segment_outside_the_arena_or_with_a_bad_size_is_not_followed(cuda):
    H = W = 16
    a, far = sc.sig_with_distance(H, W, 6 * H * W)
    sig = np.stack([a, far, a, far, a, far])
    segs = [(0, 2, H, W), (4, 3, H, W), (-1, 2, H, W), (2, 2, 0, W), (2, 2, 1 << 15, 10923), (2, 2, H, W), (5, -3, H, W)]
    cuts, dist, status = device_cuts(segs, sig, 1, cuda)
    assert status.tolist() == [0, 3, 3, 3, 3, 0, 0]
    s = np.int32(SENTINEL)
    assert cuts.tolist() == [0, 1, 0, 1, s, s] and dist.tolist() == [0, 6 * H * W, 0, 6 * H * W, s, s]     # rows 4, 5: nobody's
    cuts, _, status = device_cuts([(0, 6, H, W)], sig, 1, cuda, n_rows=5)
    assert status.tolist() == [3] and (cuts == s).all()


def test_scene_cuts_refuses_on_the_host(cuda):
    from wav2lip_amd._lib import current_stream, load, ptr
    lib = load()
    segs = torch.zeros(8, dtype=torch.int32, device=cuda)
    sig = torch.zeros((4, sc.WORDS), dtype=torch.int32, device=cuda)
    out = torch.full((16,), SENTINEL, dtype=torch.int32, device=cuda)
    s, c, d, st = current_stream(), ptr(out[:4]), ptr(out[4:8]), ptr(out[8:])
    for args in ((1, None, ptr(sig), 4, 1, c, d, st), (1, ptr(segs), None, 4, 1, c, d, st), (1, ptr(segs), ptr(sig), 4, 1, None, d, st),
                 (1, ptr(segs), ptr(sig), 4, 1, c, d, None), (0, ptr(segs), ptr(sig), 4, 1, c, d, st), (1, ptr(segs), ptr(sig), -1, 1, c, d, st),
                 (1, ptr(segs), ptr(sig), 4, 0, c, d, st), (1, ptr(segs), ptr(sig), 4, 256, c, d, st),
                 (1, ctypes.c_void_p(segs.data_ptr() + 8), ptr(sig), 4, 1, c, d, st)):
        assert lib.w2l_scene_cuts(s, *args) != 0, args
        assert lib.w2l_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
