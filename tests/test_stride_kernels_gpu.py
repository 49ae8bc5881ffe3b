"""w2l_face_rects_expand_segments (csrc/detect.hip) against the numpy model of tests/_stride_cases.py, by equality:
the rule is integers only.  Every case of a stride in one launch, the segments side by side with guard rows before, between and
after them in the key arenas and in the full arenas, empty segments among them, sentinel outputs; the status rules; every
refusal; two launches give the same bytes; and the unchanged w2l_face_boxes_runs and w2l_face_spans_segments on the expanded arenas
against their own models fed the model's expansion."""
import numpy as np
import pytest
import torch

import _noface_cases as noface
import _span_cases as spans
import _stride_cases as cases
from _noface_cases import FH, FW

pytestmark = pytest.mark.gpu

FENCE = 1000000
SENTINEL = -7
GROUPS = cases.groups()
SMALL = cases.small_groups()


class _Launch:
    """the segments of one group side by side: one guard row before, between and after them in the key arenas (flagged found,
    huge coordinates) and in the full arenas (sentinels), a segment with n <= 0 after every third one"""

    def __init__(self, cuda, group, N):
        Rk = sum(len(f) for _, _, _, f in group) + len(group) + 1
        R = sum(n for _, n, _, _ in group) + len(group) + 1
        self.key_rects, self.key_flags = np.full((Rk, 4), FENCE, np.int32), np.ones((Rk,), np.int32)
        self.segs, self.case_of, krow, row = [], [], 1, 1
        for k, (_, n, rects, flags) in enumerate(group):
            m = len(flags)
            self.key_rects[krow:krow + m], self.key_flags[krow:krow + m] = rects, flags
            self.segs.append((krow, row, n))
            self.case_of.append(k)
            if k % 3 == 0:
                self.segs.append((krow + m // 2, row + n // 2, 0 if k % 2 else -5))       # nothing to do: n <= 0
                self.case_of.append(None)
            krow, row = krow + m + 1, row + n + 1
        self.N, self.Rk, self.R, self.cuda = N, Rk, R, cuda
        self.set_table(self.segs)
        self.key_rects_dev, self.key_flags_dev = torch.from_numpy(self.key_rects).to(cuda), torch.from_numpy(self.key_flags).to(cuda)
        self.inside = np.zeros(R, bool)
        for _, row0, n in self.segs:
            self.inside[row0:row0 + max(n, 0)] = True

    def set_table(self, segs):
        from wav2lip_amd._lib import STRIDE_SEGMENT
        t = np.zeros(len(segs), STRIDE_SEGMENT)
        for k, (krow0, row0, n) in enumerate(segs):
            t[k] = (krow0, row0, n, 0)
        self.table = torch.from_numpy(t.view(np.uint8)).to(self.cuda)

    def outputs(self):
        full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=self.cuda)
        return full(self.R, 4), full(self.R), full(len(self.segs) + 1)

    def run(self, n_key_rows=None, n_rows=None):
        from wav2lip_amd import _lib
        from wav2lip_amd._lib import check, current_stream, ptr
        rects, flags, status = out = self.outputs()
        check(_lib.load().w2l_face_rects_expand_segments(current_stream(), len(self.segs), ptr(self.table), self.N, ptr(self.key_rects_dev),
                                                         ptr(self.key_flags_dev), self.Rk if n_key_rows is None else n_key_rows,
                                                         ptr(rects), ptr(flags), self.R if n_rows is None else n_rows, ptr(status)),
              "face_rects_expand_segments")
        return out


def _check_against_the_model(launch, group, out, skip=()):
    rects, flags, status = (t.cpu().numpy() for t in out)
    for k, ((_, row0, n), c) in enumerate(zip(launch.segs, launch.case_of)):
        if k in skip:
            continue
        assert status[k] == 0, k
        if c is None:
            continue
        name, n, key_rects, key_flags = group[c]
        want_rects, want_flags = cases.model(key_rects, key_flags, n, launch.N)
        assert np.array_equal(flags[row0:row0 + n], want_flags), name
        assert np.array_equal(rects[row0:row0 + n], want_rects), name
    guard = ~launch.inside
    for k in skip:
        guard[launch.segs[k][1]:launch.segs[k][1] + launch.segs[k][2]] = True
    assert (rects[guard] == SENTINEL).all() and (flags[guard] == SENTINEL).all()
    assert status[len(launch.segs)] == SENTINEL


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=["N%d" % N for N, _ in GROUPS])
def test_face_rects_expand_segments_is_the_model(cuda, g):
    N, group = GROUPS[g]
    launch = _Launch(cuda, group, N)
    out = launch.run()
    _check_against_the_model(launch, group, out)
    again = launch.run()
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(out, again))
    assert np.array_equal(launch.key_rects_dev.cpu().numpy(), launch.key_rects)            # the inputs are read only
    assert np.array_equal(launch.key_flags_dev.cpu().numpy(), launch.key_flags)


@pytest.mark.parametrize("g", range(len(SMALL)), ids=["N%d" % N for N, _ in SMALL])
def test_the_unchanged_finishes_on_the_expanded_arenas_give_their_models(cuda, g):
    """w2l_face_boxes_runs and w2l_face_spans_segments read the expanded arenas as they read the detector's: their existing models,
    fed the model's expansion, give their outputs"""
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import BOX_SEGMENT, check, current_stream, ptr
    N, group = SMALL[g]
    launch = _Launch(cuda, group, N)
    rects, flags, _ = launch.run()
    t = np.zeros(len(launch.segs), BOX_SEGMENT)
    for k, (_, row0, n) in enumerate(launch.segs):
        t[k] = (row0, n, FH, FW)
    table = torch.from_numpy(t.view(np.uint8)).to(cuda)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=cuda)
    wanted = [None if c is None else cases.model(group[c][2], group[c][3], group[c][1], N) for c in launch.case_of]
    for pads, T, hold in (((0, 10, 0, 0), 5, 2 * N - 1), ((-2, 7, 5, -3), 0, 1)):
        boxes, valid, status = full(launch.R, 4), full(launch.R), full(len(launch.segs), 2)
        check(_lib.load().w2l_face_boxes_runs(current_stream(), len(launch.segs), ptr(table), ptr(rects), ptr(flags), launch.R, *pads, T,
                                              hold, ptr(boxes), ptr(valid), ptr(status)), "face_boxes_runs")
        boxes, valid, status = boxes.cpu().numpy(), valid.cpu().numpy(), status.cpu().numpy()
        for k, ((_, row0, n), want) in enumerate(zip(launch.segs, wanted)):
            if want is None:
                assert status[k].tolist() == [0, 0]
                continue
            name = group[launch.case_of[k]][0]
            host = np.flatnonzero(want[1] == 2)
            if len(host):                                  # a flag 2 stays on its key row, where the finish meets it
                assert status[k].tolist() == [2, host[0]] and not boxes[row0:row0 + n].any() and not valid[row0:row0 + n].any(), name
                continue
            want_boxes, want_valid = noface.model(cases.filled_rects(*want), FH, FW, pads, T, hold)
            assert status[k].tolist() == [0, 0], name
            assert np.array_equal(valid[row0:row0 + n], want_valid.astype(np.int32)), (name, pads, T, hold)
            assert np.array_equal(boxes[row0:row0 + n], want_boxes), (name, pads, T, hold)
    for B, M, S in ((2 * N - 1, 1, 0), (2 * N - 2, 3, 0)):           # a missed key is bridged iff 2N - 1 <= bridge
        rects_out, flags_out, rows, status = full(launch.R, 4), full(launch.R), full(launch.R, 4), full(len(launch.segs), 2)
        check(_lib.load().w2l_face_spans_segments(current_stream(), len(launch.segs), ptr(table), ptr(rects), ptr(flags), launch.R, B, M, S,
                                                  ptr(rects_out), ptr(flags_out), ptr(rows), ptr(status)), "face_spans_segments")
        rects_out, flags_out, rows, status = (a.cpu().numpy() for a in (rects_out, flags_out, rows, status))
        for k, ((_, row0, n), want) in enumerate(zip(launch.segs, wanted)):
            if want is None:
                assert status[k].tolist() == [0, 0]
                continue
            name = group[launch.case_of[k]][0]
            want_rects, want_flags, want_rows, want_status = spans.model(want[0], want[1], B, M, S)
            assert tuple(status[k].tolist()) == want_status, (name, B)
            assert np.array_equal(flags_out[row0:row0 + n], want_flags) and np.array_equal(rects_out[row0:row0 + n], want_rects), (name, B)
            if want_rows is not None:
                assert np.array_equal(rows[row0:row0 + n], want_rows), (name, B)


def test_a_segment_outside_its_arenas_is_not_followed_and_its_neighbours_are(cuda):
    N, group = GROUPS[0]
    launch = _Launch(cuda, group, N)
    last = len(launch.segs) - 1
    assert launch.case_of[last] is not None and launch.segs[last][2] > 2
    out = launch.run(n_rows=launch.segs[last][1] + launch.segs[last][2] - 1)                   # its last row lies outside
    assert out[2][last].item() == 3
    _check_against_the_model(launch, group, out, skip=(last,))                                 # its rows still hold the sentinel
    out = launch.run(n_key_rows=launch.Rk - 2)                                                 # its last key row lies outside
    assert out[2][last].item() == 3
    _check_against_the_model(launch, group, out, skip=(last,))
    big = 0x7fffffff
    segs = [(-1, 1, 4), (1, -1, 4), (1, 2, 3), (big - 4, 2, 3), (1, big - 4, big), (1, 2, big), (launch.Rk - 1, 6, 3)]
    launch.segs, launch.case_of = segs, [None] * len(segs)
    launch.set_table(segs)
    rects, flags, status = (a.cpu().numpy() for a in launch.run())
    assert status.tolist() == [3, 3, 0, 3, 3, 3, 3, SENTINEL]
    want_rects, want_flags = cases.model(launch.key_rects[1:3], launch.key_flags[1:3], 3, N)   # N = 2: keys 0 and 2
    assert np.array_equal(rects[2:5], want_rects) and np.array_equal(flags[2:5], want_flags)
    assert (flags[:2] == SENTINEL).all() and (flags[5:] == SENTINEL).all()
    assert (rects[:2] == SENTINEL).all() and (rects[5:] == SENTINEL).all()


def test_face_rects_expand_segments_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    N, group = GROUPS[0]
    launch = _Launch(cuda, group[:4], N)
    rects, flags, status = outs = launch.outputs()
    s, n_seg = current_stream(), len(launch.segs)
    good = [ptr(launch.table), ptr(launch.key_rects_dev), ptr(launch.key_flags_dev), ptr(rects), ptr(flags), ptr(status)]

    def call(a, n_seg=n_seg, N=N, n_key_rows=launch.Rk, n_rows=launch.R):
        return lib.w2l_face_rects_expand_segments(s, n_seg, a[0], N, a[1], a[2], n_key_rows, a[3], a[4], n_rows, a[5])

    for kw in (dict(n_seg=0), dict(n_seg=-1), dict(N=0), dict(N=-2), dict(N=33), dict(n_key_rows=-1), dict(n_rows=-1)):
        assert call(good, **kw) != 0, kw
        assert b"face_rects_expand_segments" in lib.w2l_last_error(), kw
    for k in range(6):
        a = list(good)
        a[k] = None
        assert call(a) != 0 and b"NULL" in lib.w2l_last_error(), k
    for k, t in ((0, launch.table), (1, launch.key_rects_dev), (3, rects)):                    # the table and the two rect arenas
        for off in (4, 8):
            a = list(good)
            a[k] = t.data_ptr() + off
            assert call(a) != 0 and b"16-byte" in lib.w2l_last_error(), (k, off)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)                                      # nothing ran
    assert call(good, N=1) == 0 and call(good, N=32) == 0                                      # the ends of the range
    torch.cuda.synchronize()
    assert (status.cpu()[:n_seg] != SENTINEL).all()
