"""w2l_face_spans_segments (csrc/detect.hip) against the numpy model of tests/_span_cases.py, by equality: the
rule is integers only.  Every case of a parameter set in one launch, with empty segments among them and guard rows before, between
and after them; the unchanged w2l_face_boxes_runs on its outputs against the model of tests/_noface_cases.py; the status rules;
every refusal; two launches give the same bytes."""
import numpy as np
import pytest
import torch

import _noface_cases as noface
import _span_cases as cases
from _noface_cases import FH, FW

pytestmark = pytest.mark.gpu

FENCE = 1000000
SENTINEL = -7
GROUPS = cases.groups()


class _Launch:
    """the segments of one group side by side in the arenas: one guard row before, between and after them - flagged detected, with
    huge coordinates, as is the rect of every undetected row - an empty segment after every third one, sentinel outputs"""

    def __init__(self, cuda, group):
        from wav2lip_amd.face_detection import many
        R = sum(len(f) for _, _, f in group) + len(group) + 1
        self.rects, self.flags = np.full((R, 4), FENCE, np.int32), np.ones((R,), np.int32)
        self.segs, self.case_of, row = [], [], 1
        for k, (_, rects, flags) in enumerate(group):
            n = len(flags)
            self.rects[row:row + n] = np.where(flags[:, None] == 1, rects, FENCE)
            self.flags[row:row + n] = flags
            self.segs.append((row, n))
            self.case_of.append(k)
            if k % 3 == 0:
                self.segs.append((row + n // 2, 0 if k % 2 else -5))           # nothing to do: n <= 0
                self.case_of.append(None)
            row += n + 1
        self.R, self.cuda = R, cuda
        t = np.zeros(len(self.segs), many.BOX_SEGMENT)
        for k, (row0, n) in enumerate(self.segs):
            t[k] = (row0, n, 0, 0)                                             # H and W are not read
        self.table = torch.from_numpy(t.view(np.uint8)).to(cuda)
        self.rects_dev, self.flags_dev = torch.from_numpy(self.rects).to(cuda), torch.from_numpy(self.flags).to(cuda)
        self.inside = np.zeros(R, bool)
        for row0, n in self.segs:
            self.inside[row0:row0 + max(n, 0)] = True

    def outputs(self):
        full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=self.cuda)
        return full(self.R, 4), full(self.R), full(self.R, 4), full(len(self.segs) + 1, 2)

    def run(self, B, M, S, n_rows=None):
        from wav2lip_amd import _lib
        from wav2lip_amd._lib import check, current_stream, ptr
        rects_out, flags_out, spans, status = out = self.outputs()
        check(_lib.load().w2l_face_spans_segments(current_stream(), len(self.segs), ptr(self.table), ptr(self.rects_dev), ptr(self.flags_dev),
                                                  self.R if n_rows is None else n_rows, B, M, S, ptr(rects_out), ptr(flags_out),
                                                  ptr(spans), ptr(status)), "face_spans_segments")
        return out


def _check_against_the_model(launch, group, params, out, skip=()):
    rects_out, flags_out, spans, status = (t.cpu().numpy() for t in out)
    B, M, S = params
    for k, ((row0, n), c) in enumerate(zip(launch.segs, launch.case_of)):
        if k in skip:
            continue
        if c is None:
            assert status[k].tolist() == [0, 0], (params, k)
            continue
        name, rects, flags = group[c]
        want_rects, want_flags, want_spans, want_status = cases.model(rects, flags, B, M, S)
        rows = slice(row0, row0 + n)
        assert tuple(status[k].tolist()) == want_status, (params, name)
        if want_status[0] == 2:                            # left to the host: the input as it lies in the arena, no span row written
            assert np.array_equal(rects_out[rows], launch.rects[rows]) and np.array_equal(flags_out[rows], launch.flags[rows]), name
            assert (spans[rows] == SENTINEL).all(), name
            continue
        assert np.array_equal(flags_out[rows], want_flags), (params, name)
        assert np.array_equal(rects_out[rows], want_rects), (params, name)
        assert np.array_equal(spans[rows], want_spans), (params, name)
    guard = ~launch.inside
    for k in skip:
        guard[launch.segs[k][0]:launch.segs[k][0] + launch.segs[k][1]] = True
    assert (rects_out[guard] == SENTINEL).all() and (flags_out[guard] == SENTINEL).all() and (spans[guard] == SENTINEL).all()
    assert (status[len(launch.segs):] == SENTINEL).all()


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=["B%d-M%d-S%d" % p for p, _ in GROUPS])
def test_face_spans_segments_is_the_model(cuda, g):
    params, group = GROUPS[g]
    launch = _Launch(cuda, group)
    out = launch.run(*params)
    _check_against_the_model(launch, group, params, out)
    again = launch.run(*params)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(out, again))


@pytest.mark.parametrize("g", [k for k, (p, _) in enumerate(GROUPS) if p in ((25, 1, 0), (1, 4, 30), (250, 4, 30))])
def test_the_unchanged_finish_on_its_outputs_gives_the_runs_of_the_kept_spans(cuda, g):
    """w2l_face_boxes_runs with hold 0 reads rects_out / flags_out as it reads the detector's arenas: every kept span is padded,
    clipped and smoothed as a clip of its own; a segment left to the host reports the same row"""
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    from wav2lip_amd.face_detection import many
    params, group = GROUPS[g]
    launch = _Launch(cuda, group)
    rects_out, flags_out, _, _ = launch.run(*params)
    t = np.zeros(len(launch.segs), many.BOX_SEGMENT)
    for k, (row0, n) in enumerate(launch.segs):
        t[k] = (row0, n, FH, FW)
    table = torch.from_numpy(t.view(np.uint8)).to(cuda)
    for pads, T in (((0, 10, 0, 0), 5), ((-2, 7, 5, -3), 0)):
        boxes = torch.full((launch.R, 4), SENTINEL, dtype=torch.int32, device=cuda)
        valid = torch.full((launch.R,), SENTINEL, dtype=torch.int32, device=cuda)
        status = torch.full((len(launch.segs), 2), SENTINEL, dtype=torch.int32, device=cuda)
        check(_lib.load().w2l_face_boxes_runs(current_stream(), len(launch.segs), ptr(table), ptr(rects_out), ptr(flags_out), launch.R,
                                              *pads, T, 0, ptr(boxes), ptr(valid), ptr(status)), "face_boxes_runs")
        boxes, valid, status = boxes.cpu().numpy(), valid.cpu().numpy(), status.cpu().numpy()
        for k, ((row0, n), c) in enumerate(zip(launch.segs, launch.case_of)):
            if c is None:
                assert status[k].tolist() == [0, 0]
                continue
            name, rects, flags = group[c]
            want_rects, want_flags, _, want_status = cases.model(rects, flags, *params)
            if want_status[0] == 2:
                assert tuple(status[k].tolist()) == want_status and not boxes[row0:row0 + n].any() and not valid[row0:row0 + n].any()
                continue
            want, want_valid = noface.model(cases.filled_rects(want_rects, want_flags), FH, FW, pads, T, 0)
            assert status[k].tolist() == [0, 0], name
            assert np.array_equal(valid[row0:row0 + n], want_valid.astype(np.int32)), (name, pads, T)
            assert np.array_equal(boxes[row0:row0 + n], want), (name, pads, T)


def test_a_segment_outside_the_arenas_is_not_followed_and_its_neighbours_are(cuda):
    params, group = GROUPS[0]
    launch = _Launch(cuda, group)
    last = len(launch.segs) - 1
    assert launch.case_of[last] is not None and launch.segs[last][1] > 2
    out = launch.run(*params, n_rows=launch.segs[last][0] + launch.segs[last][1] - 1)          # its last row lies outside
    assert out[3][last].tolist() == [3, 0]
    _check_against_the_model(launch, group, params, out, skip=(last,))                          # its rows still hold the sentinel
    t = np.zeros(3, dtype=[("row0", np.int32), ("n", np.int32), ("H", np.int32), ("W", np.int32)])
    t[0], t[1], t[2] = (-1, 4, 0, 0), (2, 3, 0, 0), (0x7ffffff0, 0x7fffffff, 0, 0)              # row0 < 0; fine; row0 + n beyond int32
    launch.segs, launch.case_of = [(-1, 4), (2, 3), (0x7ffffff0, 0x7fffffff)], [None] * 3
    launch.table = torch.from_numpy(t.view(np.uint8)).to(cuda)
    rects_out, flags_out, spans, status = (a.cpu().numpy() for a in launch.run(0, 1, 0))
    assert status[:3].tolist() == [[3, 0], list(cases.model(launch.rects[2:5], launch.flags[2:5], 0, 1, 0)[3]), [3, 0]]
    assert (flags_out[:2] == SENTINEL).all() and (flags_out[5:] == SENTINEL).all() and (flags_out[2:5] != SENTINEL).all()
    assert (spans[:2] == SENTINEL).all() and (spans[5:] == SENTINEL).all() and (rects_out[:2] == SENTINEL).all()


def test_face_spans_segments_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    launch = _Launch(cuda, [GROUPS[0][1][0]])
    rects_out, flags_out, spans, status = outs = launch.outputs()
    s, n_seg, R = current_stream(), len(launch.segs), launch.R
    good = [ptr(launch.table), ptr(launch.rects_dev), ptr(launch.flags_dev), ptr(rects_out), ptr(flags_out), ptr(spans), ptr(status)]

    def call(a, n_seg=n_seg, n_rows=R, B=25, M=100, S=0):
        return lib.w2l_face_spans_segments(s, n_seg, a[0], a[1], a[2], n_rows, B, M, S, a[3], a[4], a[5], a[6])

    for kw in (dict(n_seg=0), dict(n_seg=-1), dict(n_rows=-1), dict(B=-1), dict(B=251), dict(M=0), dict(M=-4), dict(M=(1 << 30) + 1),
               dict(S=-1), dict(S=32768)):
        assert call(good, **kw) != 0, kw
        assert b"face_spans_segments" in lib.w2l_last_error(), kw
    for k in range(7):
        a = list(good)
        a[k] = None
        assert call(a) != 0 and b"NULL" in lib.w2l_last_error(), k
    for k, t in ((0, launch.table), (1, launch.rects_dev), (3, rects_out), (5, spans)):       # the table and the three rect arenas
        for off in (4, 8):
            a = list(good)
            a[k] = t.data_ptr() + off
            assert call(a) != 0 and b"16-byte" in lib.w2l_last_error(), (k, off)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)                                       # nothing ran
    assert call(good, B=250, M=1 << 30, S=32767) == 0 and call(good, B=0, M=1, S=0) == 0        # the ends of the ranges
    torch.cuda.synchronize()
    assert status.cpu()[:n_seg, 0].tolist() == [0] * n_seg
