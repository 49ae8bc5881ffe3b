"""The two finish kernels of the pass-through rule for frames without a face (csrc/detect.hip) against the numpy
model of tests/_noface_cases.py, by equality: integer inputs and one correctly rounded fp64 division on both sides.
w2l_face_boxes_runs on every length x flag pattern in one launch between fence rows; w2l_face_boxes_stream_runs on clips cut
into ticks six ways, many streams per launch, boxes, valid and the carry slot after every tick; the status rules; every refusal."""
import numpy as np
import pytest
import torch

import _noface_cases as cases
from _noface_cases import FH, FW

pytestmark = pytest.mark.gpu

FENCE = 1000000
SENTINEL = -7
N_SLOTS = 24
CARRY_INTS = 644


def _arena(clips):
    """the clips' rows side by side with one fence row of huge coordinates before, between and after them; an undetected row's
    rect is huge too: (rects, flags, [(row0, n)])"""
    from wav2lip_amd.face_detection.s3fd import RECT_FOUND, RECT_NONE
    R = sum(len(c) for c in clips) + len(clips) + 1
    rects, flags = np.full((R, 4), FENCE, np.int32), np.full((R,), RECT_FOUND, np.int32)
    segs, row = [], 1
    for c in clips:
        for i, r in enumerate(c):
            if r is None:
                flags[row + i] = RECT_NONE
            else:
                rects[row + i] = r
        segs.append((row, len(c)))
        row += len(c) + 1
    return rects, flags, segs


def _run_runs(cuda, rects, flags, segs, pads, T, G, n_rows=None):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    from wav2lip_amd.face_detection import many
    t = np.zeros(len(segs), many.BOX_SEGMENT)
    for k, (row0, n) in enumerate(segs):
        t[k] = (row0, n, FH, FW)
    t_dev = torch.from_numpy(t.view(np.uint8)).to(cuda)
    rects_dev, flags_dev = torch.from_numpy(rects).to(cuda), torch.from_numpy(flags).to(cuda)
    boxes = torch.full((len(rects), 4), SENTINEL, dtype=torch.int32, device=cuda)
    valid = torch.full((len(rects),), SENTINEL, dtype=torch.int32, device=cuda)
    status = torch.full((len(segs) + 1, 2), SENTINEL, dtype=torch.int32, device=cuda)
    check(_lib.load().w2l_face_boxes_runs(current_stream(), len(segs), ptr(t_dev), ptr(rects_dev), ptr(flags_dev),
                                          len(rects) if n_rows is None else n_rows, *pads, T, G, ptr(boxes), ptr(valid), ptr(status)),
          "face_boxes_runs")
    return boxes.cpu().numpy(), valid.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("G", cases.HOLDS)
@pytest.mark.parametrize("T", cases.WINDOWS)
def test_face_boxes_runs_is_the_model(cuda, T, G):
    """every length with every flag pattern, and the clips built around T and G, in one launch per pad set"""
    clips = cases.all_clips(T, G, seed=100 * T + G)
    rects, flags, segs = _arena([c for _, c in clips])
    for pads in cases.PADS:
        boxes, valid, status = _run_runs(cuda, rects, flags, segs, pads, T, G)
        assert not status[:len(segs)].any() and (status[len(segs):] == SENTINEL).all()
        inside = np.zeros(len(rects), bool)
        for (name, clip), (row0, n) in zip(clips, segs):
            want, want_valid = cases.model(clip, FH, FW, pads, T, G)
            assert np.array_equal(valid[row0:row0 + n], want_valid.astype(np.int32)), (name, pads)
            assert np.array_equal(boxes[row0:row0 + n], want), (name, pads, boxes[row0:row0 + n], want)
            inside[row0:row0 + n] = True
        assert (boxes[~inside] == SENTINEL).all() and (valid[~inside] == SENTINEL).all()      # no fence row was written
        assert np.abs(boxes[inside]).max() < 1000                                             # and none, and no undetected rect, read


def test_face_boxes_runs_equals_face_boxes_segments_on_clips_with_every_frame_detected(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    from wav2lip_amd.face_detection import many
    rng = np.random.default_rng(7)
    clips = [cases.clip_rects(np.ones(n, bool), rng) for n in cases.LENGTHS]
    rects, flags, segs = _arena(clips)
    t = np.zeros(len(segs), many.BOX_SEGMENT)
    for k, (row0, n) in enumerate(segs):
        t[k] = (row0, n, FH, FW)
    t_dev, rects_dev, flags_dev = (torch.from_numpy(a).to(cuda) for a in (t.view(np.uint8), rects, flags))
    for T in cases.WINDOWS:
        old = torch.full((len(rects), 4), SENTINEL, dtype=torch.int32, device=cuda)
        status = torch.zeros((len(segs), 2), dtype=torch.int32, device=cuda)
        check(_lib.load().w2l_face_boxes_segments(current_stream(), len(segs), ptr(t_dev), ptr(rects_dev), ptr(flags_dev), 0, 10, 0, 0, T,
                                                  ptr(old), ptr(status)), "face_boxes_segments")
        new, valid, _ = _run_runs(cuda, rects, flags, segs, (0, 10, 0, 0), T, 3)
        assert np.array_equal(new, old.cpu().numpy())
        assert all((valid[row0:row0 + n] == 1).all() for row0, n in segs)


def test_face_boxes_runs_leaves_a_clip_with_a_host_row_to_the_host_and_its_neighbours_alone(cuda):
    from wav2lip_amd.face_detection.s3fd import RECT_HOST
    T, G, pads = 5, 1, (0, 10, 0, 0)
    rng = np.random.default_rng(11)
    clips = [cases.clip_rects(rng.random(n) < 0.6, rng) for n in (9, 70, 12, 5)]
    rects, flags, segs = _arena(clips)
    flags[segs[1][0] + 66] = RECT_HOST             # inside a clip with misses, in its second chunk
    flags[segs[1][0] + 68] = 12345                 # no flag at all: the first such row is reported
    flags[segs[3][0]] = RECT_HOST
    boxes, valid, status = _run_runs(cuda, rects, flags, segs, pads, T, G)
    assert status[:4].tolist() == [[0, 0], [2, 66], [0, 0], [2, 0]]
    for k, (row0, n) in enumerate(segs):
        if status[k, 0]:
            assert not boxes[row0:row0 + n].any() and not valid[row0:row0 + n].any()
        else:
            want, want_valid = cases.model(clips[k], FH, FW, pads, T, G)
            assert np.array_equal(boxes[row0:row0 + n], want) and np.array_equal(valid[row0:row0 + n], want_valid)
        assert (boxes[row0 - 1] == SENTINEL).all() and (boxes[row0 + n] == SENTINEL).all()
    # a segment whose rows leave the arenas is not followed: status 3, nothing written
    boxes, valid, status = _run_runs(cuda, rects, flags, segs, pads, T, G, n_rows=segs[3][0] + 2)
    assert status[:4].tolist() == [[0, 0], [2, 66], [0, 0], [3, 0]]
    assert (boxes[segs[3][0]:] == SENTINEL).all() and (valid[segs[3][0]:] == SENTINEL).all()


def test_face_boxes_runs_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    from wav2lip_amd.face_detection import many
    lib = _lib.load()
    rects, flags, segs = _arena([cases.clip_rects(np.ones(4, bool), np.random.default_rng(1))])
    t = np.zeros(1, many.BOX_SEGMENT)
    t[0] = (segs[0][0], 4, FH, FW)
    t_dev, rects_dev, flags_dev = (torch.from_numpy(a).to(cuda) for a in (t.view(np.uint8), rects, flags))
    boxes = torch.full((len(rects), 4), SENTINEL, dtype=torch.int32, device=cuda)
    valid = torch.full((len(rects),), SENTINEL, dtype=torch.int32, device=cuda)
    status = torch.full((1, 2), SENTINEL, dtype=torch.int32, device=cuda)
    s = current_stream()
    for n_seg, n_rows, T, G in ((0, 6, 5, 0), (-1, 6, 5, 0), (1, -1, 5, 0), (1, 6, -1, 0), (1, 6, 65, 0), (1, 6, 5, -1), (1, 6, 5, 251)):
        assert lib.w2l_face_boxes_runs(s, n_seg, ptr(t_dev), ptr(rects_dev), ptr(flags_dev), n_rows, 0, 0, 0, 0, T, G, ptr(boxes),
                                       ptr(valid), ptr(status)) != 0
        assert b"face_boxes_runs" in lib.w2l_last_error()
    args = [ptr(t_dev), ptr(rects_dev), ptr(flags_dev), ptr(boxes), ptr(valid), ptr(status)]
    for k in range(6):
        a = list(args)
        a[k] = None
        assert lib.w2l_face_boxes_runs(s, 1, a[0], a[1], a[2], 6, 0, 0, 0, 0, 5, 0, a[3], a[4], a[5]) != 0
    assert lib.w2l_face_boxes_runs(s, 1, t_dev.data_ptr() + 4, ptr(rects_dev), ptr(flags_dev), 6, 0, 0, 0, 0, 5, 0, ptr(boxes), ptr(valid),
                                   ptr(status)) != 0 and b"16-byte" in lib.w2l_last_error()
    torch.cuda.synchronize()
    assert bool((boxes == SENTINEL).all()) and bool((valid == SENTINEL).all()) and bool((status == SENTINEL).all())      # nothing ran
    assert lib.w2l_face_boxes_runs(s, 1, ptr(t_dev), ptr(rects_dev), ptr(flags_dev), 6, 0, 0, 0, 0, 64, 250, ptr(boxes), ptr(valid),
                                   ptr(status)) == 0
    assert status.cpu().tolist() == [[0, 0]]


# ---------------------------------------------------------------- w2l_face_boxes_stream_runs
class _Tick:
    """one launch: the streams' new rows side by side in the arenas between fence rows, output rows with a sentinel row between
    the segments, sentinel status rows behind the real ones"""

    def __init__(self, cuda, parts, T, carry):
        """parts: [(new rects or None per frame, slot, seen, closed)]"""
        from wav2lip_amd.face_detection import live
        self.rects, self.flags, rows = _arena([p[0] for p in parts])
        self.segs = np.zeros(len(parts), live.BOX_STREAM_SEGMENT)
        out = 1
        for k, ((new, slot, seen, closed), (row0, n)) in enumerate(zip(parts, rows)):
            lo, hi = cases.tick_range(seen, seen + n, closed, T)
            self.segs[k] = (row0, n, FH, FW, slot, seen, int(closed), out)
            out += hi - lo + 1
        self.n_out, self.T, self.cuda, self.carry = out, T, cuda, carry
        self.boxes = torch.full((out, 4), SENTINEL, dtype=torch.int32, device=cuda)
        self.valid = torch.full((out,), SENTINEL, dtype=torch.int32, device=cuda)
        self.status = torch.full((len(parts) + 2, 2), SENTINEL, dtype=torch.int32, device=cuda)

    def launch(self, pads, G, n_seg=None, T=None, segs_dev=None, null=None, n_slots=N_SLOTS, expect_ok=True):
        from wav2lip_amd import _lib
        from wav2lip_amd._lib import current_stream, ptr
        lib = _lib.load()
        self.segs_dev = torch.from_numpy(self.segs.view(np.uint8).copy()).to(self.cuda)
        self.rects_dev, self.flags_dev = torch.from_numpy(self.rects).to(self.cuda), torch.from_numpy(self.flags).to(self.cuda)
        args = [self.segs.ctypes.data, ptr(self.segs_dev) if segs_dev is None else segs_dev, ptr(self.rects_dev), ptr(self.flags_dev),
                ptr(self.carry), ptr(self.boxes), ptr(self.valid), ptr(self.status)]
        if null is not None:
            args[null] = None
        rc = lib.w2l_face_boxes_stream_runs(current_stream(), len(self.segs) if n_seg is None else n_seg, args[0], args[1], args[2],
                                            args[3], len(self.rects), args[4], n_slots, *pads, self.T if T is None else T, G, args[5],
                                            args[6], self.n_out, args[7])
        torch.cuda.synchronize()
        if expect_ok:
            assert rc == 0, lib.w2l_last_error()
        else:
            assert rc != 0 and b"face_boxes_stream_runs" in lib.w2l_last_error()
        return self.boxes.cpu().numpy(), self.valid.cpu().numpy(), self.status.cpu().numpy()

    def check_fences(self, boxes, valid, status, written):
        """`written`: [(out0, count)] of the segments that wrote; every other output row and the spare status rows are sentinels"""
        inside = np.zeros(len(boxes), bool)
        for out0, count in written:
            inside[out0:out0 + count] = True
        assert (boxes[~inside] == SENTINEL).all() and (valid[~inside] == SENTINEL).all()
        assert (status[len(self.segs):] == SENTINEL).all()
        assert np.abs(boxes[inside]).max(initial=0) < 1000                       # no fence row and no undetected rect was read


def _new_carry(cuda):
    return torch.full((N_SLOTS, CARRY_INTS), SENTINEL, dtype=torch.int32, device=cuda)


def _check_carry(carry, states, used):
    """a stream's slot starts with its last min(n, 2 max(T, 1)) rows and holds the distance from the last detection at word 640;
    slots that belong to nobody are untouched"""
    got = carry.cpu().numpy()
    for slot, (rows, dist) in states.items():
        assert np.array_equal(got[slot, :rows.size].reshape(-1, 5), rows), slot
        assert got[slot, 640] == dist, (slot, got[slot, 640], dist)
    assert (got[[s for s in range(N_SLOTS) if s not in used]] == SENTINEL).all()


@pytest.mark.parametrize("kind", ["whole", "1", "T-1", "T", "seeded", "seeded, closed empty"])
@pytest.mark.parametrize("T,G,pads", [(T, G, cases.PADS[(i + j) % 2]) for i, T in enumerate(cases.WINDOWS) for j, G in enumerate(cases.HOLDS)])
def test_face_boxes_stream_runs_is_the_model_tick_by_tick(cuda, kind, T, G, pads):
    """all streams of a tick in one launch; per tick boxes, valid and the carry are the model's, and over all ticks a stream's
    boxes are the whole-clip model's however it was cut"""
    rng = np.random.default_rng(1000 * T + 10 * G + len(kind))
    clips = cases.stream_clips(T, G, seed=3 + 100 * T + G)
    videos = [c for _, c in clips]
    slots = [2 * k + 1 for k in range(len(videos))][:N_SLOTS // 2] + [2 * k for k in range(len(videos) - N_SLOTS // 2)]
    ticks = [cases.cuts(kind, len(v), T, rng) for v in videos]
    carry = _new_carry(cuda)
    states, pos = {}, [0] * len(videos)
    got, got_valid = [[] for _ in videos], [[] for _ in videos]
    for t in range(max(len(c) for c in ticks)):
        live_now = [k for k in range(len(videos)) if t < len(ticks[k])]
        parts = [(videos[k][pos[k]:pos[k] + ticks[k][t]], slots[k], pos[k], t == len(ticks[k]) - 1) for k in live_now]
        table = _Tick(cuda, parts, T, carry)
        boxes, valid, status = table.launch(pads, G)
        assert not status[:len(parts)].any()
        written = []
        for (new, slot, seen, closed), seg, k in zip(parts, table.segs, live_now):
            want, want_valid, states[slot] = cases.model_tick(videos[k][:seen + len(new)], seen, closed, FH, FW, pads, T, G)
            out0 = int(seg["out0"])
            assert np.array_equal(valid[out0:out0 + len(want)], want_valid.astype(np.int32)), (clips[k][0], t, seen, len(new), closed)
            assert np.array_equal(boxes[out0:out0 + len(want)], want), (clips[k][0], t, seen, len(new), closed)
            written.append((out0, len(want)))
            got[k].append(want)
            got_valid[k].append(want_valid)
            pos[k] += len(new)
        table.check_fences(boxes, valid, status, written)
        _check_carry(carry, states, set(slots))
    for k, video in enumerate(videos):
        want, want_valid = cases.model(video, FH, FW, pads, T, G)
        assert np.array_equal(np.concatenate(got[k]), want) and np.array_equal(np.concatenate(got_valid[k]), want_valid)


def test_face_boxes_stream_runs_leaves_a_stream_with_a_host_row_as_it_was(cuda):
    from wav2lip_amd.face_detection.s3fd import RECT_HOST
    T, G, pads = 5, 2, (0, 10, 0, 0)
    rng = np.random.default_rng(5)
    carry = _new_carry(cuda)
    first = [cases.clip_rects(rng.random(n) < 0.7, rng) for n in (6, 3, 70)]
    table = _Tick(cuda, [(r, k + 1, 0, False) for k, r in enumerate(first)], T, carry)
    table.launch(pads, G)
    before = carry.cpu().numpy().copy()
    second = [cases.clip_rects(rng.random(n) < 0.7, rng) for n in (4, 70, 9)]
    table = _Tick(cuda, [(r, k + 1, len(first[k]), k == 2) for k, r in enumerate(second)], T, carry)
    table.flags[int(table.segs[1]["row0"]) + 66] = RECT_HOST
    table.flags[int(table.segs[1]["row0"]) + 68] = 12345
    boxes, valid, status = table.launch(pads, G)
    assert status[:3].tolist() == [[0, 0], [2, 3 + 66], [0, 0]]
    written = []
    for k in (0, 2):
        want, want_valid, _ = cases.model_tick(first[k] + second[k], len(first[k]), k == 2, FH, FW, pads, T, G)
        out0 = int(table.segs[k]["out0"])
        assert np.array_equal(boxes[out0:out0 + len(want)], want) and np.array_equal(valid[out0:out0 + len(want)], want_valid)
        assert len(want) > 0
        written.append((out0, len(want)))
    table.check_fences(boxes, valid, status, written)                             # no box of stream 1 was written
    assert np.array_equal(carry.cpu().numpy()[2], before[2])                      # and its carry is left as it was


def test_face_boxes_stream_runs_refuses_bad_arguments_without_launching(cuda):
    rng = np.random.default_rng(2)
    carry = _new_carry(cuda)
    parts = [(cases.clip_rects(np.ones(6, bool), rng), 1, 0, False), (cases.clip_rects(np.ones(3, bool), rng), 2, 0, True)]

    def refused(edit=None, **kw):
        table = _Tick(cuda, parts, 5, carry)
        if edit is not None:
            edit(table)
        boxes, valid, status = table.launch((0, 10, 0, 0), kw.pop("G", 0), expect_ok=False, **kw)
        assert (boxes == SENTINEL).all() and (valid == SENTINEL).all() and (status == SENTINEL).all()      # nothing ran

    for null in range(8):
        refused(null=null)
    for kw in (dict(n_seg=0), dict(T=65), dict(T=-1), dict(G=-1), dict(G=251), dict(n_slots=0), dict(n_slots=2)):
        refused(**kw)

    def field(k, name, value):
        def edit(table):
            table.segs[k][name] = value
        return edit

    for edit in (field(0, "n_new", -1), field(0, "seen", -1), field(1, "slot", 1), field(0, "slot", -1), field(0, "row0", -1),
                 field(1, "row0", 10), field(0, "out0", -1), field(1, "out0", 2), field(1, "out0", 10)):
        refused(edit)
    table = _Tick(cuda, parts, 5, carry)
    refused(segs_dev=0)
    table.segs_dev = torch.zeros(80, dtype=torch.uint8, device=cuda)
    refused(segs_dev=table.segs_dev.data_ptr() + 4)
    assert (carry.cpu().numpy() == SENTINEL).all()
    # the kernel does not follow a device table that disagrees with the checked host copy: status 3, nothing else written
    table = _Tick(cuda, parts, 5, carry)
    wrong = table.segs.copy()
    wrong[0]["slot"] = N_SLOTS
    wrong[1]["row0"] = 1 << 20
    wrong_dev = torch.from_numpy(wrong.view(np.uint8)).to(cuda)
    boxes, valid, status = table.launch((0, 10, 0, 0), 0, segs_dev=wrong_dev.data_ptr())
    assert status[:2].tolist() == [[3, 0], [3, 0]]
    assert (boxes == SENTINEL).all() and (valid == SENTINEL).all() and (carry.cpu().numpy() == SENTINEL).all()
