"""w2l_s3fd_top_rects and w2l_face_track_segments (csrc/detect.hip; tracked face selection) against the model of
tests/_track_cases.py: exact equality everywhere, guard bands around every output, hand-made cases for each edge of the rule and
random ones that are checked not to be vacuous."""

import numpy as np
import pytest
import torch

import _track_cases as tc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A5A5A5A            # ints on either side of an output (256 bytes: the 16-byte alignments survive)


def guarded(n, dev):
    """(the whole tensor, the n ints in its middle) of an int32 buffer filled with the sentinel"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all())


def device_top(table, keep, counts, K, dev, scale=(1.0, 1.0)):
    """w2l_s3fd_top_rects called directly, outputs between guard bands -> numpy (cands [B,K,4], ncand [B], flags [B])"""
    from wav2lip_amd._lib import check, current_stream, load, ptr
    B, P = table.shape[:2]
    t, k, c = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (table, keep, counts))
    (wc, cands), (wn, ncand), (wf, flags) = guarded(B * K * 4, dev), guarded(B, dev), guarded(B, dev)
    check(load().w2l_s3fd_top_rects(current_stream(), B, P, ptr(t), ptr(k), ptr(c), 0.5, float(scale[0]), float(scale[1]), K, ptr(cands),
                                    ptr(ncand), ptr(flags)), "s3fd_top_rects")
    assert guards_intact(wc) and guards_intact(wn) and guards_intact(wf)
    return cands.cpu().numpy().reshape(B, K, 4), ncand.cpu().numpy(), flags.cpu().numpy()


def check_top(table, keep, counts, K, dev, scale=(1.0, 1.0)):
    """the device against the model for every image; returns the device's three arrays"""
    table, keep, counts = np.asarray(table, np.float32), np.asarray(keep, np.int32), np.asarray(counts, np.int32)
    cands, ncand, flags = device_top(table, keep, counts, K, dev, scale)
    for b in range(len(table)):
        want, flag = tc.model_top_rects(table[b], keep[b], counts[b], K, *scale)
        assert flags[b] == flag and ncand[b] == len(want), (b, flags[b], flag, ncand[b], want)
        assert cands[b, :len(want)].tolist() == [list(r) for r in want], (b, cands[b], want)
        assert not cands[b, len(want):].any(), b                                   # unused slots are zeros
    return cands, ncand, flags


def one_image(rows, order=None):
    """table [1, P, 5] of `rows` and a keep list over them (default: row order)"""
    t = np.asarray(rows, np.float32).reshape(1, -1, 5)
    k = np.asarray(order if order is not None else range(t.shape[1]), np.int32)
    keep = np.zeros((1, t.shape[1]), np.int32)
    keep[0, :len(k)] = k
    return t, keep, np.asarray([len(k)], np.int32)


def passing(i):
    return [10 + i, 20 + i, 30 + 2 * i, 40 + 3 * i, 0.6 + 0.001 * i]


FAILING = [1, 1, 2, 2, 0.4]


# ---------------------------------------------------------------- w2l_s3fd_top_rects
@pytest.mark.parametrize("K", [1, 3, 16])
def test_exactly_k_one_more_and_no_passing_rows(cuda, K):
    for n_pass in (K, K + 1, 0, K - 1):
        rows = []
        for i in range(n_pass):
            rows += [FAILING] * (i % 3) + [passing(i)]
        rows += [FAILING] * 2
        cands, ncand, flags = check_top(*one_image(rows), K, cuda)
        assert ncand[0] == min(n_pass, K) and flags[0] == (tc.FOUND if n_pass else tc.NONE)
        if n_pass:
            assert cands[0, 0].tolist() == [10, 20, 30, 40]


@pytest.mark.parametrize("first", [63, 64, 200])
def test_a_passing_row_at_the_wave_boundaries_and_beyond_three_chunks(cuda, first):
    rows = [FAILING] * first + [passing(0)] + [FAILING] * 70 + [passing(1), passing(2)]
    cands, ncand, flags = check_top(*one_image(rows), 2, cuda)
    assert ncand[0] == 2 and cands[0].tolist() == [[10, 20, 30, 40], [11, 21, 32, 43]]
    cands, ncand, _ = check_top(*one_image(rows), 8, cuda)
    assert ncand[0] == 3
    # the K-th passing row is the last lane of a chunk; the next chunk opens with a bad entry that must not be looked at
    rows = [FAILING] * 62 + [passing(0), passing(1)] + [FAILING]
    t, keep, n = one_image(rows)
    keep[0, 64] = 1000
    assert check_top(t, keep, n, 2, cuda)[2][0] == tc.FOUND and check_top(t, keep, n, 3, cuda)[2][0] == tc.HOST


def test_a_bad_row_index_flags_the_frame_only_up_to_the_kth_passing_row(cuda):
    rows = [passing(0), FAILING, passing(1), FAILING, passing(2), FAILING]
    for bad in (-1, 6, 2 ** 31 - 1, -2 ** 31):
        for at in range(6):
            t, keep, n = one_image(rows)
            keep[0, at] = bad
            for K in (1, 2, 3, 4):
                # passing rows sit at 0, 2, 4: the K-th is at 2K - 2 (K = 4: there is none, every entry is examined)
                flagged = at <= 2 * K - 2 or K == 4
                cands, ncand, flags = check_top(t, keep, n, K, cuda)
                assert (flags[0] == tc.HOST) == flagged, (bad, at, K)
                if flagged:
                    assert ncand[0] == 0 and not cands.any()


@pytest.mark.parametrize("coord", range(4))
def test_coordinates_the_device_does_not_convert_and_the_ones_at_the_bound(cuda, coord):
    from wav2lip_amd.face_detection.s3fd import first_rects
    for value, flagged in ((np.nan, True), (np.inf, True), (32767.0, False), (32767.996, False), (32768.0, True), (3e9, True),
                           (-5.5, False), (-np.inf, False), (-0.0, False)):
        row = passing(1)
        row[coord] = value
        t, keep, n = one_image([passing(0), row, passing(2)])
        cands, ncand, flags = check_top(t, keep, n, 3, cuda)
        assert (flags[0] == tc.HOST) == flagged, (value, flags)
        if not flagged:
            assert ncand[0] == 3 and cands[0, 1, coord] == (32767 if value > 0 else 0)
        # the row is not looked at after the K-th passing row
        assert check_top(t, keep, n, 1, cuda)[2][0] == tc.FOUND
        # as candidate 0 it is what first_rect converts, wherever both decide
        t0, keep0, n0 = one_image([row, passing(2)])
        c0, _, f0 = check_top(t0, keep0, n0, 2, cuda)
        fr = first_rects(*(torch.from_numpy(x).to(cuda) for x in (t0, keep0, n0)), 0.5)
        if f0[0] == tc.FOUND:
            assert fr[0, 4] == tc.FOUND and fr[0, :4].tolist() == c0[0, 0].tolist()
        else:
            assert fr[0, 4] == tc.HOST or value in (32768.0,)


def test_a_count_that_is_not_final_is_left_to_the_host(cuda):
    t, keep, _ = one_image([passing(0), passing(1)])
    t, keep = np.repeat(t, 4, axis=0), np.repeat(keep, 4, axis=0)
    cands, ncand, flags = check_top(t, keep, np.array([-1, 3, 2, 0], np.int32), 4, cuda)
    assert flags.tolist() == [tc.HOST, tc.HOST, tc.FOUND, tc.NONE] and ncand.tolist() == [0, 0, 2, 0]


def test_a_scaled_frame_gives_the_bits_of_scale_box_then_int(cuda):
    from wav2lip_amd.face_detection.s3fd import det_rect_scale, scale_box
    r = np.random.default_rng(3)
    rows = np.concatenate([r.uniform(-20, 700, (1, 300, 4)), r.uniform(0.3, 1.0, (1, 300, 1))], axis=2).astype(np.float32)
    keep = np.arange(300, dtype=np.int32)[None]
    n = np.array([300], np.int32)
    for scale in (det_rect_scale(1080, 1920, 360, 640), det_rect_scale(721, 1283, 103, 183), (np.float32(1.0), np.float32(7.0))):
        cands, ncand, flags = check_top(rows, keep, n, 16, cuda, scale)
        assert flags[0] == tc.FOUND and ncand[0] == 16
        taken = [i for i in range(300) if rows[0, i, 4] > 0.5][:16]
        want = [[int(v) for v in np.maximum(scale_box(rows[0, i, :4], *scale), 0)] for i in taken]
        assert cands[0].tolist() == want
    unscaled = check_top(rows, keep, n, 16, cuda)[0]
    assert unscaled.tolist() == check_top(rows, keep, n, 16, cuda, (np.float32(1), np.float32(1)))[0].tolist()
    # a product above the bound flags the frame although the coordinate itself is below it
    big = one_image([[10, 10, 20000, 50, 0.9]])
    assert check_top(*big, 1, cuda)[2][0] == tc.FOUND and check_top(*big, 1, cuda, (2.0, 1.0))[2][0] == tc.HOST


@pytest.fixture(scope="module")
def random_nms(cuda):
    """B = 64 random tables of P = 1500 rows through the device NMS, computed once: (table, keep, counts) as numpy"""
    from wav2lip_amd.face_detection.s3fd import first_rects, nms_batch
    r = np.random.default_rng(64)
    B, P = 64, 1500
    xy = r.normal(80, 60, (B, P, 2))
    wh = r.uniform(2, 90, (B, P, 2))
    sc = r.uniform(0, 1, (B, P)) * r.uniform(0.3, 1.05, (B, 1))          # some images with no score above 0.5
    t = np.concatenate([xy, xy + wh, sc[..., None]], axis=2).astype(np.float32)
    tab = torch.from_numpy(t).to(cuda)
    keep, counts = nms_batch(tab, 0.05, 0.3)
    first = first_rects(tab, keep, counts, 0.5)
    return t, keep.cpu().numpy(), counts.cpu().numpy(), first


@pytest.mark.parametrize("K", [1, 8, 16])
def test_random_tables_through_the_device_nms(cuda, random_nms, K):
    t, keep, counts, first = random_nms
    cands, ncand, flags = check_top(t, keep, counts, K, cuda)
    assert 0 < (flags == tc.FOUND).sum() < len(t) and (flags != tc.HOST).all()
    assert (ncand <= K).all() and (K == 1 or (ncand > 1).any())
    both = (flags == tc.FOUND) & (first[:, 4] == tc.FOUND)
    assert both.sum() == (flags == tc.FOUND).sum() and (cands[both, 0] == first[both, :4]).all()
    assert ((flags == tc.NONE) == (first[:, 4] == tc.NONE)).all()


def test_the_wrapper_brings_everything_back_in_one_copy(cuda, random_nms):
    from wav2lip_amd.face_detection.s3fd import top_rects
    t, keep, counts, _ = random_nms
    got = top_rects(*(torch.from_numpy(x).to(cuda) for x in (t[:5], keep[:5], counts[:5])), 0.5, 4)
    want = device_top(t[:5], keep[:5], counts[:5], 4, cuda)
    assert all(g.dtype == np.int32 and (g == w).all() for g, w in zip(got, want)) and got[0].shape == (5, 4, 4)
    with pytest.raises(RuntimeError, match="K=17"):
        top_rects(*(torch.from_numpy(x).to(cuda) for x in (t[:5], keep[:5], counts[:5])), 0.5, 17)


# ---------------------------------------------------------------- w2l_face_track_segments
def device_track(dev, segs, cands, ncand, cflags, K, pick, L, q, state=None):
    """w2l_face_track_segments called directly, outputs between guard bands.  segs: [(row0, n, slot, seen)]; state: numpy int32
    [slots, 8] or None.  Returns numpy (rects [R,4], flags [R], status [n_seg], the state table afterwards or None); rows no
    segment names keep the sentinel."""
    from wav2lip_amd._lib import TRACK_SEGMENT, check, current_stream, load, ptr
    R = len(ncand)
    table = np.zeros(len(segs), dtype=TRACK_SEGMENT)
    for k, s in enumerate(segs):
        table[k] = s
    segs_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
    c, n, f = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in (cands, ncand, cflags))
    (wr, rects), (wf, flags), (ws, status) = guarded(R * 4, dev), guarded(R, dev), guarded(len(segs), dev)
    wst = st = None
    if state is not None:
        wst, st = guarded(state.size, dev)
        st.copy_(torch.from_numpy(np.ascontiguousarray(state, dtype=np.int32).reshape(-1)).to(dev))
    check(load().w2l_face_track_segments(current_stream(), len(segs), ptr(segs_dev), ptr(c), ptr(n), ptr(f), R, K, tc.PICKS.index(pick), L,
                                         q, ptr(st), 0 if state is None else len(state), ptr(rects), ptr(flags), ptr(status)),
          "face_track_segments")
    assert guards_intact(wr) and guards_intact(wf) and guards_intact(ws) and (wst is None or guards_intact(wst))
    return (rects.cpu().numpy().reshape(R, 4), flags.cpu().numpy(), status.cpu().numpy(),
            None if state is None else st.cpu().numpy().reshape(state.shape))


def check_clips(dev, clips, K, pick, L, q):
    """every clip a segment of one launch (no carried state), against the model; returns the model's events per clip"""
    clips = [[(c[:K], f) for c, f in clip] for clip in clips]         # a candidate beyond K is not there at all
    frames = [f for clip in clips for f in clip]
    segs, r = [], 0
    for clip in clips:
        segs.append((r, len(clip), -1, 0))
        r += len(clip)
    rects, flags, status, _ = device_track(dev, segs, *tc.pack_frames(frames, K), K, pick, L, q)
    assert not status.any()
    events = []
    for (row0, n, _, _), clip in zip(segs, clips):
        want_r, want_f, _, ev = tc.model_track(clip, pick, L, q)
        assert flags[row0:row0 + n].tolist() == want_f.tolist(), (row0, flags[row0:row0 + n], want_f)
        assert rects[row0:row0 + n].tolist() == want_r.tolist(), row0
        events.append(ev)
    return rects, flags, events


def found(*cands):
    return (list(cands), tc.FOUND)


NO_FACE = ([], tc.NONE)
A, B_ = (10, 10, 30, 30), (50, 12, 72, 34)         # two faces, well apart


def moved(r, d):
    return (r[0] + d, r[1], r[2] + d, r[3])


def test_two_faces_whose_scores_swap_every_other_frame(cuda):
    """the defining case: candidate 0 alternates between the two heads, the tracked rect stays on one"""
    clip = [found(moved(A, i), moved(B_, i)) if i % 2 == 0 else found(moved(B_, i), moved(A, i)) for i in range(12)]
    untracked = [c[0] for c, _ in clip]
    assert untracked[0] == A and untracked[1] == moved(B_, 1)
    for pick, face in (("score", A), ("left", A), ("right", B_), ("largest", B_)):
        rects, flags, _ = check_clips(cuda, [clip], 8, pick, 0, 64)
        assert rects.tolist() == [list(moved(face, i)) for i in range(12)] and (flags == tc.FOUND).all()
    rects, _, _ = check_clips(cuda, [clip], 1, "score", 0, 64)        # K = 1 is the untracked rule
    assert rects.tolist() == [list(r) for r in untracked]


def test_each_pick_and_its_ties_go_to_the_lower_index(cuda):
    small, large, large2 = (40, 40, 50, 50), (0, 0, 30, 20), (60, 5, 80, 35)              # areas 100, 600, 600; x1 + x2 = 90, 30, 140
    same_left, same_right = (5, 50, 25, 60), (65, 50, 75, 60)                              # x1 + x2 = 30 and 140 again
    frame = found(small, large, large2, same_left, same_right)
    want = {"score": small, "largest": large, "left": large, "right": large2}
    for pick, rect in want.items():
        rects, _, ev = check_clips(cuda, [[frame]], 8, pick, 0, 64)
        assert rects[0].tolist() == list(rect) and (pick == "score" or "seed_tie" in ev[0][0])
    # the same candidates in another order: the tie goes to whichever comes first
    frame = found(same_right, same_left, large2, large, small)
    for pick, rect in {"score": same_right, "largest": large2, "left": same_left, "right": same_right}.items():
        assert check_clips(cuda, [[frame]], 8, pick, 0, 64)[0][0].tolist() == list(rect)
    # a candidate beyond K is not there at all, and candidate 15 of 16 can win
    many = [(i, 0, i + 10, 10) for i in range(15)] + [(100, 0, 300, 10)]
    assert check_clips(cuda, [[found(*many)]], 16, "largest", 0, 64)[0][0].tolist() == [100, 0, 300, 10]
    assert check_clips(cuda, [[found(*many)]], 16, "right", 0, 64)[0][0].tolist() == [100, 0, 300, 10]


def test_an_iou_tie_goes_to_the_lower_index(cuda):
    ref = (20, 20, 40, 40)
    left, right = (10, 20, 30, 40), (30, 20, 50, 40)            # both overlap ref by half: inter 200, union 600
    for order in ((left, right), (right, left)):
        rects, _, ev = check_clips(cuda, [[found(ref), found(*order)]], 4, "score", 0, 64)
        assert rects[1].tolist() == list(order[0]) and "iou_tie" in ev[0][1]
    # equal IoU from different (inter, union): 2/4 against 1/2 in cross-multiplied form
    a, b = (20, 20, 40, 30), (20, 20, 30, 40)                    # inter 200 each, area 200: union 400
    c = (20, 20, 40, 60)                                         # inter 400, union 800
    rects, _, ev = check_clips(cuda, [[found(ref), found(c, a, b)]], 4, "score", 0, 64)
    assert rects[1].tolist() == list(c) and "iou_tie" in ev[0][1]
    rects, _, _ = check_clips(cuda, [[found(ref), found(b, c, a)]], 4, "score", 0, 64)
    assert rects[1].tolist() == list(b)
    # a strictly larger IoU wins from any slot
    better = (21, 20, 41, 40)
    for slot in range(4):
        cands = [left, right, a]
        cands.insert(slot, better)
        assert check_clips(cuda, [[found(ref), found(*cands)]], 4, "score", 0, 64)[0][1].tolist() == list(better)


@pytest.mark.parametrize("q", [1, 64, 128, 255, 256])
def test_the_threshold_continues_at_equality_and_not_one_pixel_below(cuda, q):
    """ref 256 x 1 and a candidate of q x 1 inside it: inter = q, union = 256, so inter * 256 == q * union exactly"""
    ref, other = (0, 0, 256, 1), (100, 100, 120, 120)
    at, below = (0, 0, q, 1), (0, 0, q - 1, 1)
    assert tc.inter_union(at, ref) == (q, 256) and tc.inter_union(below, ref) == (q - 1, 256)
    rects, flags, ev = check_clips(cuda, [[found(ref), found(other, at)]], 4, "score", 0, q)
    assert rects[1].tolist() == list(at) and "continue" in ev[0][1]
    rects, flags, ev = check_clips(cuda, [[found(ref), found(other, below)]], 4, "score", 0, q)
    assert rects[1].tolist() == list(other) and "reseed" in ev[0][1]         # lost at L = 0: seeded again on the same frame
    rects, flags, ev = check_clips(cuda, [[found(ref), found(other, below)]], 4, "score", 1, q)
    assert flags[1] == tc.NONE and not rects[1].any()


def test_touching_rects_and_zero_area_rects(cuda):
    ref = (10, 10, 20, 20)
    touching = [(20, 10, 30, 20), (10, 20, 20, 30), (20, 20, 30, 30), (0, 10, 10, 20)]         # inter = 0 on an edge or a corner
    for t in touching:
        rects, flags, ev = check_clips(cuda, [[found(ref), found(t)]], 2, "score", 1, 1)
        assert flags[1] == tc.NONE and "miss" in ev[0][1]
    line, point = (12, 10, 12, 20), (15, 15, 15, 15)               # zero area inside ref: inter = 0, never an overlap
    rects, flags, ev = check_clips(cuda, [[found(ref), found(line, point)]], 2, "score", 1, 1)
    assert flags[1] == tc.NONE
    # but zero-area candidates are kept, seed a track, and are never continued - not even by themselves
    rects, flags, ev = check_clips(cuda, [[found(point), found(point), found(line, ref)]], 2, "largest", 0, 1)
    assert rects.tolist() == [list(point), list(point), list(ref)] and "reseed" in ev[0][1] and "reseed" in ev[0][2]
    # a rect with a negative side never overlaps either, whatever its "area"
    rects, flags, _ = check_clips(cuda, [[found(ref), found((20, 20, 10, 10), (18, 12, 12, 18))]], 2, "score", 5, 1)
    assert flags[1] == tc.NONE


@pytest.mark.parametrize("L", [0, 1, 3])
def test_the_frame_on_which_the_track_is_seeded_again(cuda, L):
    far = (200, 200, 230, 230)
    clip = [found(A)] + [found(far)] * 6
    rects, flags, ev = check_clips(cuda, [clip], 2, "score", L, 64)
    assert flags.tolist() == [tc.FOUND] + [tc.NONE] * L + [tc.FOUND] * (6 - L)
    assert "reseed" in ev[0][L + 1] and all("reseed" not in e for e in ev[0][:L + 1])
    # the face comes back on the last tolerated frame: the count starts again
    clip = [found(A)] + [found(far)] * L + [found(far, A)] + [found(far)] * L + [found(A, far)]
    rects, flags, _ = check_clips(cuda, [clip], 2, "score", L, 64)
    assert flags.tolist() == [tc.FOUND] + [tc.NONE] * L + [tc.FOUND] + [tc.NONE] * L + [tc.FOUND]
    assert rects[L + 1].tolist() == list(A) and rects[-1].tolist() == list(A)
    # frames without any candidate count as missed ones, and seed nothing
    clip = [found(A)] + [NO_FACE] * (L + 2) + [found(far)]
    rects, flags, _ = check_clips(cuda, [clip], 2, "score", L, 64)
    assert flags.tolist() == [tc.FOUND] + [tc.NONE] * (L + 2) + [tc.FOUND] and rects[-1].tolist() == list(far)


def test_a_frame_left_to_the_host_leaves_the_state_alone(cuda):
    far = (200, 200, 230, 230)
    host, garbage = ([], tc.HOST), ([], 7)                         # a word that is no flag at all counts as one too
    clip = [found(A), found(far), host, garbage, found(far), found(far, A)]
    rects, flags, _ = check_clips(cuda, [clip], 2, "score", 2, 64)
    assert flags.tolist() == [tc.FOUND, tc.NONE, tc.HOST, tc.HOST, tc.NONE, tc.FOUND] and rects[5].tolist() == list(A)
    # the candidates a flagged row happens to hold are not read as candidates
    cands, ncand, cflags = tc.pack_frames([found(A), found(far), found(A)], 2)
    cflags[1] = tc.HOST
    rects, flags, status, _ = device_track(cuda, [(0, 3, -1, 0)], cands, ncand, cflags, 2, "score", 0, 64)
    assert flags.tolist() == [tc.FOUND, tc.HOST, tc.FOUND] and not rects[1].any()
    # a count beyond K, or a negative one, is cut to the table
    cands, ncand, cflags = tc.pack_frames([found(A, far), found(far, A)], 2)
    ncand[:] = (99, -3)
    rects, flags, _, _ = device_track(cuda, [(0, 2, -1, 0)], cands, ncand, cflags, 2, "right", 0, 64)
    assert rects[0].tolist() == list(far) and flags.tolist() == [tc.FOUND, tc.NONE]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_clip_lengths_around_one_wave(cuda, n):
    rng = np.random.default_rng(n)
    clip = tc.random_clip(rng, n, 5, p_host=0.05)
    for pick in tc.PICKS:
        check_clips(cuda, [clip], 5, pick, 1, 64)


def test_seventy_segments_of_mixed_length_in_one_launch(cuda):
    rng = np.random.default_rng(70)
    clips = [tc.random_clip(rng, int(n), 7, p_host=0.02) for n in rng.integers(0, 90, 70)]
    clips[3], clips[69] = [], tc.random_clip(rng, 130, 7)
    for pick, L in (("score", 0), ("largest", 2), ("right", 5)):
        check_clips(cuda, clips, 7, pick, L, 64)


def test_a_bad_segment_is_not_followed_and_its_neighbours_are(cuda):
    rng = np.random.default_rng(9)
    frames = tc.random_clip(rng, 40, 4)
    arenas = tc.pack_frames(frames, 4)
    state = rng.integers(-50, 50, (3, 8)).astype(np.int32)
    good = [(0, 10, -1, 0), (30, 10, -1, 0)]
    for bad in ((10, 31, -1, 0), (-1, 5, -1, 0), (15, -1, -1, 0), (39, 2, -1, 0), (12, 5, 3, 0), (12, 5, -2, 0), (12, 5, 1, -1),
                (2 ** 31 - 1, 2 ** 31 - 1, -1, 0)):
        rects, flags, status, after = device_track(cuda, [good[0], bad, good[1]], *arenas, 4, "left", 1, 64, state)
        assert status.tolist() == [0, 3, 0], bad
        assert (after == state).all()
        for row0, n, _, _ in good:
            want_r, want_f, _, _ = tc.model_track(frames[row0:row0 + n], "left", 1, 64)
            assert rects[row0:row0 + n].tolist() == want_r.tolist() and flags[row0:row0 + n].tolist() == want_f.tolist()
        untouched = np.r_[10:30]
        assert (rects[untouched] == SENTINEL).all() and (flags[untouched] == SENTINEL).all()
    # without a state table every slot but -1 is outside it
    _, _, status, _ = device_track(cuda, [(0, 5, 0, 0), (5, 5, -1, 0)], *arenas, 4, "left", 1, 64)
    assert status.tolist() == [3, 0]


def run_in_pieces(dev, frames, cuts, K, pick, L, q, slot, state):
    """the frames through slot `slot` of `state`, one launch per piece; returns (rects, flags, the state table at the end)"""
    rects, flags, seen = [], [], 0
    for a, b in zip([0] + cuts, cuts + [len(frames)]):
        piece = frames[a:b]
        arenas = tc.pack_frames(piece, K) if piece else (np.zeros((1, K, 4), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32))
        r, f, status, state = device_track(dev, [(0, len(piece), slot, seen)], *arenas, K, pick, L, q, state)
        assert status.tolist() == [0]
        rects += r[:len(piece)].tolist()
        flags += f[:len(piece)].tolist()
        seen += len(piece)
    return rects, flags, state


def test_every_two_way_cut_of_twelve_frames_through_a_slot_equals_one_launch(cuda):
    rng = np.random.default_rng(12)
    for case in range(6):
        pick, L = tc.PICKS[case % 4], (0, 1, 3)[case % 3]
        frames = tc.random_clip(rng, 12, 4, hi=30, p_host=0.1)
        want_r, want_f, words, _ = tc.model_track(frames, pick, L, 64)
        garbage = rng.integers(-9, 99, (4, 8)).astype(np.int32)    # seen = 0: what the slot held before is not read
        for cut in range(0, 13):
            rects, flags, state = run_in_pieces(cuda, frames, [cut], 4, pick, L, 64, 2, garbage.copy())
            assert rects == want_r.tolist() and flags == want_f.tolist(), (case, cut)
            assert state[2].tolist() == list(words) and (state[[0, 1, 3]] == garbage[[0, 1, 3]]).all(), (case, cut)


def test_random_cuts_of_two_hundred_frames_through_a_slot_equal_one_launch(cuda):
    rng = np.random.default_rng(200)
    for case in range(4):
        pick, L = tc.PICKS[case], (0, 1, 3, 7)[case]
        frames = tc.random_clip(rng, 200, 6, p_host=0.03)
        want_r, want_f, words, ev = tc.model_track(frames, pick, L, 64)
        assert any("miss" in e and "lost" not in e for e in ev) or L == 0      # states with a count in them are carried
        for _ in range(3):
            cuts = sorted(rng.integers(0, 201, int(rng.integers(2, 12))).tolist())
            garbage = rng.integers(-9, 99, (5, 8)).astype(np.int32)
            rects, flags, state = run_in_pieces(cuda, frames, cuts, 6, pick, L, 64, 4, garbage.copy())
            assert rects == want_r.tolist() and flags == want_f.tolist(), (case, cuts)
            assert state[4].tolist() == list(words) and (state[:4] == garbage[:4]).all()


def test_two_streams_in_one_launch_keep_their_own_slots(cuda):
    rng = np.random.default_rng(2)
    a, b = tc.random_clip(rng, 30, 4), tc.random_clip(rng, 30, 4)
    state = np.zeros((3, 8), np.int32)
    state[1] = 77
    out = {0: ([], []), 2: ([], [])}
    for lo, hi in ((0, 7), (7, 8), (8, 30)):
        frames = a[lo:hi] + b[lo:hi]
        n = hi - lo
        r, f, status, state = device_track(cuda, [(0, n, 0, lo), (n, n, 2, lo)], *tc.pack_frames(frames, 4), 4, "largest", 2, 64, state)
        assert not status.any() and (state[1] == 77).all()
        for slot, row0 in ((0, 0), (2, n)):
            out[slot][0].extend(r[row0:row0 + n].tolist())
            out[slot][1].extend(f[row0:row0 + n].tolist())
    for slot, clip in ((0, a), (2, b)):
        want_r, want_f, words, _ = tc.model_track(clip, "largest", 2, 64)
        assert out[slot][0] == want_r.tolist() and out[slot][1] == want_f.tolist() and state[slot].tolist() == list(words)


@pytest.mark.parametrize("pick", tc.PICKS)
def test_three_hundred_random_clips(cuda, pick):
    rng = np.random.default_rng(300 + tc.PICKS.index(pick))
    K = 6
    clips = [tc.random_clip(rng, int(rng.integers(1, 41)), K) for _ in range(300)]
    happened = set()
    for L, q in ((0, 64), (1, 64), (3, 26), (0, 256), (2, 1)):
        _, _, events = check_clips(cuda, clips, K, pick, L, q)
        happened |= {word for ev in events for e in ev for word in e}
    assert happened >= {"continue", "iou_tie", "miss", "lost", "reseed", "seed", "none"}, happened
    assert pick == "score" or "seed_tie" in happened


def test_coordinates_at_the_bound_stay_exact(cuda):
    """rects as large as w2l_s3fd_top_rects lets through: the products reach 2^60 and must not wrap"""
    m = tc.MAX_COORD
    ref = (0, 0, m, m)
    near = [(0, 0, m, m - 1), (0, 0, m - 1, m), (1, 0, m, m), (0, 1, m, m)]        # IoU (m - 1) / m each: 255/256 < it < 1
    for order in (near + [ref], [ref] + near, near[2:] + [ref] + near[:2]):
        rects, _, _ = check_clips(cuda, [[found(ref), found(*order)]], 8, "left", 0, 256)
        assert rects[1].tolist() == [0, 0, m, m]
    for order in (near, near[::-1], near[1:] + near[:1]):
        rects, _, ev = check_clips(cuda, [[found(ref), found(*order)]], 8, "right", 0, 255)
        assert rects[1].tolist() == list(order[0]) and "iou_tie" in ev[0][1] and "continue" in ev[0][1]
        rects, _, ev = check_clips(cuda, [[found(ref), found(*order)]], 8, "largest", 3, 256)
        assert not rects[1].any() and "miss" in ev[0][1]
