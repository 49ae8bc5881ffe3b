"""Many clips through the generator in shared batches: the loop of the reference's evaluation/gen_videos_from_filelist.py
(:205-227, one clip at a time, every clip a ragged batch of its own) with the rows of successive clips packed into full batches.

Frames are independent given the weights, so a batch may hold rows of several clips.  A row is one generator
input: (frame of its clip, face box, first mel column).  Rows are appended across clip boundaries until a batch holds
`batch_size` of them - only the very last batch of a run is ragged - so the model builds plans for at most two batch sizes
per lane whatever the clip lengths, every batch but the last runs the committed launch configurations of `batch_size`, and
`LIPSYNC_DEPTH` batches are in flight from the first clip to the last.

Per batch (`BatchRunner.submit`): the (clip, frame) pairs the batch touches are deduplicated and staged in ONE pinned buffer
(staging.py lays it out) together with the two row tables (w2l_frame_row / w2l_mel_row, include/w2l_hip.h), copied to the device
once, then on the lane's
stream  w2l_crop_resize_rows_u8 -> w2l_datagen_pack -> w2l_mel_gather_rows -> the plan -> w2l_frames_to_u8 (fp32 only) ->
w2l_compose_rows_u8,  and the composed frames come back in one copy.  Frames of different clips may have different shapes.

A clip's frames may already be on the device (`ClipJob.frames` a contiguous uint8 tensor [F,H,W,3]; real_videos_inference.py
resizes and detects there): such a job stages nothing - a row's `src` is the address of the frame where it lies, only the two
tables travel up, and the outputs come back as for any other job.

`rows_inference` / `rows_filelist` are the two row conventions of the reference (inference.py:231-240 and
gen_videos_from_filelist.py:176-198); the packer knows nothing about either.
"""
import collections

import numpy as np

from ._lib import FRAME_ROW, MEL_ROW
from .inference import LIPSYNC_DEPTH, mel_chunk_starts, mel_step_size, validate_boxes
from .staging import Staging, align

ClipJob = collections.namedtuple("ClipJob", "key frames mel rows")
ClipJob.__doc__ = """one clip: `frames` uint8 [H,W,3] BGR frames (one shape per clip; a list or an [F,H,W,3] array, or a contiguous uint8
device tensor [F,H,W,3] that is read where it lies), `mel` the device [80,T] spectrogram (audio.melspectrogram_device), `rows` a list
of (frame_index, (y1, y2, x1, x2), mel_start); a row whose box is None (a frame without a face under `no_face_hold`, DESIGN.md 3v)
runs no generator row: its output frame is the frame itself"""


def rows_inference(n_mel, n_frames, boxes, fps=25., static=False):
    """rows of inference.py:231-240 + :108-131: one row per mel chunk at `fps`, the tail window re-anchored at the end, chunk i
    on frame i % n_frames (frame 0 when static) with that frame's box; a box that is None (a gap frame) stays None"""
    starts = mel_chunk_starts(n_mel, fps)
    idx = [0 if static else i % n_frames for i in range(len(starts))]
    return [(j, _box(boxes[j]), s) for j, s in zip(idx, starts)]


def _box(box):
    return None if box is None else tuple(int(v) for v in box)


def filelist_chunk_starts(n_mel):
    """gen_videos_from_filelist.py:176-183: start column of every FULL 16-column window at 25 fps; no tail window"""
    mel_idx_multiplier = 80. / 25
    starts = []
    i = 0
    while True:
        start_idx = int(i * mel_idx_multiplier)
        if start_idx + mel_step_size > n_mel:
            return starts
        starts.append(start_idx)
        i += 1


def rows_filelist(n_mel, n_frames, boxes):
    """rows of gen_videos_from_filelist.py:176-198 + :82-95: chunk i on frame i, frames truncated to the chunk count.  A clip
    with fewer frames than chunks is not runnable (:195 skips it): ValueError"""
    starts = filelist_chunk_starts(n_mel)
    if n_frames < len(starts):
        raise ValueError("%d frames for %d mel chunks: the video is shorter than its audio" % (n_frames, len(starts)))
    return [(i, _box(boxes[i]), s) for i, s in enumerate(starts)]


class _Job:
    """a ClipJob while rows of it are undelivered"""

    def __init__(self, job, n_rows):
        self.key, self.frames, self.mel, self.n_rows, self.delivered = job.key, job.frames, job.mel, n_rows, 0
        self.closed_after = []       # keys of zero-row jobs that follow this one: closed right after it, in job order

    def release(self):
        self.frames = self.mel = None


def _resident(frames):
    """True for a frame tensor (torch, [F,H,W,3]) rather than a sequence of host frames: what its shape and its checks go by
    (whether anything of it is staged is `Staging.place`'s question)"""
    return hasattr(frames, "data_ptr")


def _frame_hw(job, fi):
    f = job.frames
    return (int(f.shape[1]), int(f.shape[2])) if _resident(f) else np.asarray(f[fi]).shape[:2]


def _frame_bytes(job, fi):
    if _resident(job.frames):
        H, W = _frame_hw(job, fi)
        return H * W * 3
    return np.asarray(job.frames[fi]).nbytes


def _reserve(st, rows, n):
    """a batch of `rows` launched as n >= len(rows) rows, reserved in the Staging `st`: [frame-row table][mel-row table]
    [deduplicated host frames]; frames of a device-resident job are not in it.  Returns the handles (frame-row table, mel-row table,
    {(id(job), frame): the row's source frame})"""
    ft, mt, src = st.table(FRAME_ROW, n), st.table(MEL_ROW, n), {}
    for job, fi, _, _ in rows:
        if (id(job), fi) not in src:
            src[(id(job), fi)] = st.place(job.frames, fi)
    return ft, mt, src


def _output_layout(rows):
    """([output offset per row], output bytes): the outputs have a buffer of their own, every frame on a 16-byte boundary"""
    out_off, out_bytes = [], 0
    for job, fi, _, _ in rows:
        out_off.append(out_bytes)
        out_bytes = align(out_bytes + _frame_bytes(job, fi))
    return out_off, out_bytes


def staging_layout(rows, n):
    """where everything of a batch of `rows` launched as n >= len(rows) rows lies: (bytes of the staging buffer, offset of the
    mel-row table, {(id(job), frame): offset of a staged host frame}, [(offset, host frame)], [output offset per row], output
    bytes) - `_reserve` and `_output_layout`, nothing allocated"""
    st = Staging("cpu")
    _, mt, src = _reserve(st, rows, n)
    src_off = {k: h.offset for k, h in src.items() if h.resident is None}
    return (st.size, mt.offset, src_off, [(h.offset, f) for h, f in st.placed]) + _output_layout(rows)


class BatchRunner:
    """the device side of the packer: `submit(rows)` stages, launches and starts the copy back of one packed batch on the
    next lane and returns a ticket, `result(ticket)` waits for it and returns one uint8 [H,W,3] array per row.
    rows: [(job, frame_index, (y1, y2, x1, x2), mel_start)]; `job` is anything with `.frames`, and with `.mel` where
    `mel_start` is a column of it.  A row may name its spectrogram itself instead: `mel_start` = (device tensor [80,T], T,
    start relative to that tensor) - a stream's spectrogram window (wav2lip_amd/streaming.py).
    `submit(rows, pad_to=m)` launches m >= len(rows) rows: the last row repeated with a scratch destination, so that a ragged
    batch runs a plan of a committed size; the padded rows' outputs are dropped."""

    def __init__(self, model, batch_size, depth, precision, blend=None, color_match=None):
        import torch
        from .inference import PipelinedRunner, _blend_kw, _color_kw, _precision_kw
        self.torch = torch
        self.runner = PipelinedRunner(model, batch_size, depth=depth, **_precision_kw(precision), **_blend_kw(blend),
                                      **_color_kw(color_match))
        self.device = self.runner.lanes[0].device

    def submit(self, rows, pad_to=None):
        torch = self.torch
        real = len(rows)
        n = max(real, pad_to or 0)
        out_off, out_bytes = _output_layout(rows)
        st = Staging(self.device)
        frame_rows, mel_rows, src = _reserve(st, rows, n)
        st.allocate()
        scratch = 0
        if n > real:                             # one scratch frame behind the outputs for the padded rows
            scratch = align(_frame_bytes(rows[-1][0], rows[-1][1]))
        dev_out = torch.empty(out_bytes + scratch, dtype=torch.uint8, device=self.device)
        host_out = torch.empty(out_bytes, dtype=torch.uint8, pin_memory=True)
        src = {k: st.address(h) for k, h in src.items()}     # a resident frame's own address: read where it lies
        ft, mt = st.view(frame_rows), st.view(mel_rows)
        shapes, mels, max_px = [], {}, 1             # mels: every spectrogram the lane reads
        for r, (job, fi, (y1, y2, x1, x2), start) in enumerate(rows):
            H, W = _frame_hw(job, fi)
            ft[r] = (src[(id(job), fi)], dev_out.data_ptr() + out_off[r], H, W, y1, y2, x1, x2, (0, 0))
            mel, T, start = start if isinstance(start, tuple) else (job.mel, job.mel.shape[1], start)
            mt[r] = (mel.data_ptr(), T, start)
            mels[id(mel)] = mel
            shapes.append((H, W))
            max_px = max(max_px, H * W)
        # padding: the last row again, composed into the scratch frame.  All padded rows write that one frame at the same time,
        # and all write the same bytes (the same row), so the overlap is harmless
        ft[real:], mt[real:] = ft[real - 1], mt[real - 1]
        ft["dst"][real:] = dev_out.data_ptr() + out_bytes
        # the lane keeps the spectrograms and the resident frame tensors alive
        ticket = self.runner.submit(None, rows=(n, st.tensor(frame_rows), st.tensor(mel_rows), max_px), upload=(st.dev, st.host),
                                    download=(host_out, dev_out[:out_bytes] if scratch else dev_out),
                                    keep=tuple(mels.values()) + st.residents)
        return ticket, host_out, out_off, shapes

    def result(self, item):
        (_, done), host_out, out_off, shapes = item
        done.synchronize()                       # the copy back is part of the lane's work: wait on the host, then read
        buf = host_out.numpy()
        return [buf[o:o + h * w * 3].reshape(h, w, 3).copy() for o, (h, w) in zip(out_off, shapes)]

    @staticmethod
    def ready(item):
        """True when `result(item)` would not wait"""
        return item[0][1].query()


def _checked_rows(job):
    """the job's rows with every box, frame number and mel window validated; a ValueError names the job"""
    rows = []
    T = int(job.mel.shape[1])
    if _resident(job.frames):
        return _checked_rows_resident(job, T)
    for fi, box, start in job.rows:
        fi, start = int(fi), int(start)
        try:
            if not 0 <= fi < len(job.frames):
                raise ValueError("frame index %d outside the clip's %d frames" % (fi, len(job.frames)))
            f = job.frames[fi]
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("frames must be uint8 [H,W,3] arrays, got %s %s" % (f.dtype, f.shape))
            if start < 0 or start + mel_step_size > T:
                raise ValueError("mel window [%d, %d) outside the %d columns of the spectrogram" % (start, start + mel_step_size, T))
            if box is not None:
                box = validate_boxes([box], f.shape[0], f.shape[1])[0]
        except ValueError as e:
            raise ValueError("job %r: %s" % (job.key, e)) from None
        rows.append((fi, box, start))
    return rows


def _checked_rows_resident(job, T):
    """`_checked_rows` for a frame tensor on the device: shapes and flags only, nothing that waits for the device"""
    f = job.frames
    rows = []
    try:
        if str(f.dtype) != "torch.uint8" or f.dim() != 4 or f.shape[3] != 3 or not f.is_contiguous():
            raise ValueError("a frame tensor must be contiguous uint8 [F,H,W,3], got %s %s" % (f.dtype, tuple(f.shape)))
        F, H, W = (int(v) for v in f.shape[:3])
        for fi, box, start in job.rows:
            fi, start = int(fi), int(start)
            if not 0 <= fi < F:
                raise ValueError("frame index %d outside the clip's %d frames" % (fi, F))
            if start < 0 or start + mel_step_size > T:
                raise ValueError("mel window [%d, %d) outside the %d columns of the spectrogram" % (start, start + mel_step_size, T))
            rows.append((fi, None if box is None else validate_boxes([box], H, W)[0], start))
    except ValueError as e:
        raise ValueError("job %r: %s" % (job.key, e)) from None
    return rows


def lipsync_many(model, jobs, batch_size=128, depth=None, precision="f32", sink=None, blend=None, color_match=None):
    """Run every `ClipJob` of the iterable `jobs` (consumed lazily) through the generator, rows packed across job boundaries
    into batches of `batch_size` (only the last one ragged) on `depth` (default LIPSYNC_DEPTH) lanes.

    Every output frame (the row's frame with the generated mouth region pasted into its box) goes to `sink(key, frame_u8)` in
    row order within its job, and `sink(key, None)` follows a job's last frame; jobs finish in the order they came.  Without a
    sink the frames are collected and returned as {key: [frames]}.  Memory is bounded whatever the number of jobs: a job's
    frames and mel are released when its last row has been delivered, and the jobs alive at any time are those the rows of at
    most `depth + 1` batches touch, plus the one being read.  `blend`: None (the reference's paste) or (feather, top), every
    row's face blended into its frame (`inference.check_blend`, w2l_compose_blend_rows_u8).  `color_match`: None, "mean" or
    "full", every row's prediction matched to its crop before the paste (`inference.check_color_match`, w2l_color_match_u8).

    A row whose box is None takes no batch row: `sink` receives its frame's own bytes (copied back from the device for a
    resident job) in its place in the row order, as soon as the rows before it have been delivered."""
    from .inference import _blend_kw, _color_kw
    from .models.wav2lip import check_precision
    check_precision(precision)
    paste_kw = dict(_blend_kw(blend), **_color_kw(color_match))
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    depth = depth or LIPSYNC_DEPTH
    collected = None
    if sink is None:
        collected = {}

        def sink(key, frame):
            lst = collected.setdefault(key, [])
            if frame is not None:
                lst.append(frame)

    runner = None
    pending = collections.deque()      # (ticket, [(job, None) per row, (job, frame) per pass-through row behind it]), oldest first
    batch, order = [], []              # rows of the batch being filled; its entry of `pending` to be
    last = None                        # the newest job with undelivered rows

    def finish(job):
        job.release()
        sink(job.key, None)
        for key in job.closed_after:
            sink(key, None)

    def deliver(job, frame):
        sink(job.key, frame)
        job.delivered += 1
        if job.delivered == job.n_rows:
            finish(job)

    def source_frame(job, fi):
        f = job.frames[fi]
        return f.cpu().numpy() if _resident(job.frames) else np.array(f)

    def collect():
        item, owners = pending.popleft()
        generated = iter(runner.result(item))
        for job, fi in owners:
            deliver(job, next(generated) if fi is None else source_frame(job, fi))

    def flush():
        nonlocal batch, order
        pending.append((runner.submit(batch), order))
        batch, order = [], []
        if len(pending) >= depth:
            collect()

    def pass_through(job, fi):
        """in row order: behind the rows of the batch being filled, else behind the newest batch in flight, else at once"""
        if batch:
            order.append((job, fi))
        elif pending:
            pending[-1][1].append((job, fi))
        else:
            deliver(job, source_frame(job, fi))

    for cj in jobs:
        rows = _checked_rows(cj)
        if runner is None:
            runner = BatchRunner(model, batch_size, depth, precision, **paste_kw)
        if not rows:                                   # nothing to run: closed in job order
            if last is not None and last.delivered < last.n_rows:
                last.closed_after.append(cj.key)
            else:
                sink(cj.key, None)
            continue
        job = last = _Job(cj, len(rows))
        del cj
        for fi, box, start in rows:
            if box is None:
                pass_through(job, fi)
                continue
            batch.append((job, fi, box, start))
            order.append((job, None))
            if len(batch) == batch_size:
                flush()
    if batch:
        flush()
    while pending:
        collect()
    return collected
