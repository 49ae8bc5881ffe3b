"""w2l_face_tracks_all_segments (csrc/detect.hip; every face of a shot) against the model of tests/_faces_cases.py:
exact equality of all three outputs, guard rows around every arena, the hand-made cases for each edge of the rule (checked not to
be vacuous) and random ones at every K and F; then F = 1 against w2l_face_track_segments, and the unchanged span and run launches
over the expanded segment table against their own models per slot."""

import ctypes

import numpy as np
import pytest
import torch

import _faces_cases as fc
import _noface_cases as noface
import _span_cases as sc
import _track_cases as tc
from _noface_cases import FH, FW

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 3                                       # guard rows before, between and after the segments of a launch


class Launch:
    """the segments side by side in the candidate arenas, `GUARD` rows between them whose candidates would seed tracks if they were
    read, an empty segment after every third one; every output filled with the sentinel"""

    def __init__(self, dev, F, K, segments, extra=()):
        from wav2lip_amd._lib import BOX_SEGMENT
        self.F, self.K, self.dev = F, K, dev
        R = sum(len(s) for s in segments) + GUARD * (len(segments) + 1)
        guard = fc.found(*[(5 * c, 0, 5 * c + 30, 30) for c in range(K)])
        frames, self.segs, self.case_of = [guard] * GUARD, [], []
        for k, seg in enumerate(segments):
            self.segs.append((len(frames), len(seg)))
            self.case_of.append(k)
            if k % 3 == 0:
                self.segs.append((len(frames) + len(seg) // 2, 0))
                self.case_of.append(None)
            frames += list(seg) + [guard] * GUARD
        for e in extra:
            self.segs.append(e)
            self.case_of.append("extra")
        assert len(frames) == R
        self.R, self.frames = R, frames
        self.arenas = fc.pack(frames, K)
        t = np.zeros(len(self.segs), BOX_SEGMENT)
        for k, (row0, n) in enumerate(self.segs):
            t[k] = (row0, n, 0, 0)                              # H and W are not read
        self.table = torch.from_numpy(t.view(np.uint8)).to(dev)
        self.arenas_dev = [torch.from_numpy(a).to(dev) for a in self.arenas]
        self.inside = np.zeros(R, bool)
        for (row0, n), c in zip(self.segs, self.case_of):
            if c != "extra":
                self.inside[row0:row0 + n] = True

    def run(self, L, q):
        from wav2lip_amd._lib import check, current_stream, load, ptr
        full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=self.dev)
        rects, flags, status = full(self.F + 2, self.R, 4), full(self.F + 2, self.R), full(len(self.segs) + 2, 4)
        check(load().w2l_face_tracks_all_segments(current_stream(), len(self.segs), ptr(self.table), *(ptr(a) for a in self.arenas_dev),
                                                  self.R, self.K, self.F, L, q, ptr(rects[1]), ptr(flags[1]), ptr(status[1])),
              "face_tracks_all_segments")
        self.raw = (rects, flags, status)
        rects, flags, status = (t.cpu().numpy() for t in self.raw)
        for whole in (rects, flags, status):                    # the block before and the block after the outputs
            assert (whole[0] == SENTINEL).all() and (whole[-1] == SENTINEL).all()
        assert (rects[1:-1, ~self.inside] == SENTINEL).all() and (flags[1:-1, ~self.inside] == SENTINEL).all()
        return rects[1:-1], flags[1:-1], status[1:-1]

    def check(self, L, q):
        """all three outputs of every segment against the model; returns the model's events per segment"""
        rects, flags, status = self.run(L, q)
        events = []
        for k, ((row0, n), c) in enumerate(zip(self.segs, self.case_of)):
            if c is None:
                assert status[k].tolist() == [0, 0, 0, 0], k
                continue
            if c == "extra":
                continue
            rows = slice(row0, row0 + n)
            want_r, want_f, want_s, ev = fc.model_faces(*(a[rows] for a in self.arenas), self.F, L, q)
            assert status[k].tolist() == [0] + list(want_s), (k, status[k], want_s)
            assert np.array_equal(flags[:, rows], want_f), k
            assert np.array_equal(rects[:, rows], want_r), k
            events.append(ev)
        return events


@pytest.mark.parametrize("name", list(fc.CASES))
def test_a_hand_made_case_is_the_model(cuda, name):
    F, K, L, q, frames, must, counts = fc.CASES[name]
    launch = Launch(cuda, F, K, [frames])
    ev = launch.check(L, q)[0]
    assert must <= set().union(*ev), (name, ev)
    _, _, status = launch.run(L, q)
    assert counts is None or tuple(status[0][1:].tolist()) == counts


def test_best_pair_first_is_not_slot_order(cuda):
    F, K, L, q, frames, _, _ = fc.CASES["crossing"]
    launch = Launch(cuda, F, K, [frames])
    rects, flags, _ = launch.run(L, q)
    row = launch.segs[0][0] + 1
    assert rects[:, row].tolist() == [list(fc.Y), list(fc.X)] and flags[:, row].tolist() == [1, 1]
    other = fc.model_faces(*fc.pack(frames, K), F, L, q, slot_order=True)[0]
    assert other[:, 1].tolist() == [list(fc.X), list(fc.Y)]


RANDOM = fc.random_cases()


@pytest.mark.parametrize("g", range(len(RANDOM)), ids=["F%d-K%d-L%d-q%d" % c[:4] for c in RANDOM])
def test_random_segments_of_every_length_in_one_launch(cuda, g):
    """eight segments and three empty ones in one launch, guard rows between them; twice, with equal bytes"""
    F, K, L, q, segments = RANDOM[g]
    launch = Launch(cuda, F, K, segments)
    events = launch.check(L, q)
    seen = set().union(*[e for ev in events for e in ev])
    assert {"host", "match", "miss", "seed"} <= seen, seen
    first = [t.cpu().numpy().tobytes() for t in launch.raw]
    launch.run(L, q)
    assert first == [t.cpu().numpy().tobytes() for t in launch.raw]


def test_every_kind_of_event_occurs_in_the_random_cases():
    seen = set()
    for F, K, L, q, segments in RANDOM:
        for seg in segments:
            for ev in fc.model_faces(*fc.pack(seg, K), F, L, q)[3]:
                seen |= ev
    assert seen == {"host", "match", "tie_slot", "tie_cand", "miss", "freed", "seed", "reseed", "drop"}


@pytest.mark.parametrize("K,L,q", [(1, 0, 64), (3, 1, 1), (16, 25, 256), (8, 250, 64)])
def test_one_slot_is_the_single_track_with_pick_score(cuda, K, L, q):
    """F = 1 against a launch of w2l_face_track_segments over the same arenas, byte for byte"""
    from wav2lip_amd._lib import TRACK_SEGMENT, check, current_stream, load, ptr
    rng = np.random.default_rng([K, L, q])
    launch = Launch(cuda, 1, K, [fc.random_case(rng, n, K) for n in fc.LENGTHS])
    rects, flags, status = launch.run(L, q)
    t = np.zeros(len(launch.segs), TRACK_SEGMENT)
    for k, (row0, n) in enumerate(launch.segs):
        t[k] = (row0, n, -1, 0)
    table = torch.from_numpy(t.view(np.uint8)).to(cuda)
    one_r = torch.full((launch.R, 4), SENTINEL, dtype=torch.int32, device=cuda)
    one_f = torch.full((launch.R,), SENTINEL, dtype=torch.int32, device=cuda)
    one_s = torch.full((len(launch.segs),), SENTINEL, dtype=torch.int32, device=cuda)
    check(load().w2l_face_track_segments(current_stream(), len(launch.segs), ptr(table), *(ptr(a) for a in launch.arenas_dev), launch.R, K,
                                         0, L, q, None, 0, ptr(one_r), ptr(one_f), ptr(one_s)), "face_track_segments")
    assert not one_s.cpu().numpy().any() and not status[:, 0].any()
    assert rects[0].tobytes() == one_r.cpu().numpy().tobytes() and flags[0].tobytes() == one_f.cpu().numpy().tobytes()
    for row0, n in [s for s, c in zip(launch.segs, launch.case_of) if c is not None]:
        frames = [(list(c[:K]), f) for c, f, *_ in launch.frames[row0:row0 + n]]
        want_r, want_f, _, _ = tc.model_track(frames, "score", L, q)
        assert np.array_equal(rects[0, row0:row0 + n], want_r) and np.array_equal(flags[0, row0:row0 + n], want_f)


def test_the_unchanged_span_and_run_launches_follow_the_expanded_table(cuda):
    """w2l_face_spans_segments and w2l_face_boxes_runs (hold 0) over F * n_seg segments (t * R + row0, n, H, W) on the F slot
    arenas: every slot of every segment is its own models' answer; a segment with a host frame reports it in every slot"""
    from wav2lip_amd._lib import BOX_SEGMENT, check, current_stream, load, ptr
    from wav2lip_amd.face_detection.faces import expand_segments
    F, K, L, q = 3, 4, 2, 64
    rng = np.random.default_rng(5)
    launch = Launch(cuda, F, K, [fc.random_case(rng, n, K, hi=30, p_host=0.0 if n != 65 else 0.05, p_none=0.3) for n in fc.LENGTHS])
    launch.run(L, q)
    rects, flags = launch.raw[0][1:-1].contiguous(), launch.raw[1][1:-1].contiguous()
    R, n_seg = launch.R, len(launch.segs)
    wide = expand_segments([(row0, n, FH, FW) for row0, n in launch.segs], F, R)
    assert len(wide) == F * n_seg and wide[2 * n_seg + 1] == (2 * R + launch.segs[1][0], launch.segs[1][1], FH, FW)
    t = np.zeros(len(wide), BOX_SEGMENT)
    for k, s in enumerate(wide):
        t[k] = s
    table = torch.from_numpy(t.view(np.uint8)).to(cuda)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=cuda)
    rects2, flags2, span_rows, span_status = full(F * R, 4), full(F * R), full(F * R, 4), full(F * n_seg, 2)
    boxes, valid, status = full(F * R, 4), full(F * R), full(F * n_seg, 2)
    B, M, S, pads, T = 2, 3, 4, (0, 10, 0, 0), 5
    check(load().w2l_face_spans_segments(current_stream(), F * n_seg, ptr(table), ptr(rects), ptr(flags), F * R, B, M, S, ptr(rects2),
                                         ptr(flags2), ptr(span_rows), ptr(span_status)), "face_spans_segments")
    check(load().w2l_face_boxes_runs(current_stream(), F * n_seg, ptr(table), ptr(rects2), ptr(flags2), F * R, *pads, T, 0, ptr(boxes),
                                     ptr(valid), ptr(status)), "face_boxes_runs")
    boxes, valid, status, span_rows, span_status = (x.cpu().numpy() for x in (boxes, valid, status, span_rows, span_status))
    kept = hosts = 0
    for t_ in range(F):
        for k, ((row0, n), c) in enumerate(zip(launch.segs, launch.case_of)):
            if c is None or n == 0:
                assert span_status[t_ * n_seg + k].tolist() == [0, 0]
                continue
            rows = slice(row0, row0 + n)
            want_r, want_f, _, _ = fc.model_faces(*(a[rows] for a in launch.arenas), F, L, q)
            r2, f2, want_rows, want_status = sc.model(want_r[t_], want_f[t_], B, M, S)
            out = slice(t_ * R + row0, t_ * R + row0 + n)
            assert tuple(span_status[t_ * n_seg + k].tolist()) == want_status
            if want_status[0] == 2:
                hosts += 1
                assert tuple(status[t_ * n_seg + k].tolist()) == want_status
                continue
            kept += want_status[1]
            assert np.array_equal(span_rows[out], want_rows)
            want_b, want_v = noface.model(sc.filled_rects(r2, f2), FH, FW, pads, T, 0)
            assert np.array_equal(valid[out], want_v.astype(np.int32)) and np.array_equal(boxes[out], want_b)
    assert kept >= 6 and hosts == F


def test_a_segment_outside_the_arenas_is_not_followed_and_its_neighbours_are(cuda):
    F, K, L, q = 2, 3, 1, 64
    rng = np.random.default_rng(11)
    segments = [fc.random_case(rng, n, K) for n in (5, 9)]
    R = 5 + 9 + 3 * GUARD
    bad = [(-1, 3), (R - 2, 3), (2, -1), (0, R + 1), (2 ** 31 - 2, 5)]
    launch = Launch(cuda, F, K, segments, extra=bad)
    assert launch.R == R
    launch.check(L, q)                                          # the neighbours, and nothing outside them written
    status = launch.run(L, q)[2]
    assert status[-len(bad):].tolist() == [[3, 0, 0, 0]] * len(bad)


def test_the_launcher_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1024, dtype=torch.int32, device=cuda)
    base = buf.data_ptr()
    assert base % 16 == 0

    def go(n_seg=1, segs=base, cands=base, ncand=base, cflags=base, n_rows=4, K=8, F=4, L=0, q=64, rects=base, flags=base, status=base):
        vp = lambda v: None if v is None else ctypes.c_void_p(v)
        return lib.w2l_face_tracks_all_segments(None, n_seg, vp(segs), vp(cands), vp(ncand), vp(cflags), n_rows, K, F, L, q, vp(rects),
                                                vp(flags), vp(status))

    for kw in (dict(K=0), dict(K=17), dict(F=0), dict(F=17), dict(L=-1), dict(L=251), dict(q=0), dict(q=257), dict(n_seg=0), dict(n_rows=-1),
               dict(segs=None), dict(cands=None), dict(ncand=None), dict(cflags=None), dict(rects=None), dict(flags=None), dict(status=None),
               dict(segs=base + 4), dict(cands=base + 8), dict(rects=base + 4), dict(F=16, n_rows=1 << 25), dict(F=1, n_rows=1 << 29)):
        assert go(**kw) != 0 and b"face_tracks_all_segments" in lib.w2l_last_error(), kw
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
