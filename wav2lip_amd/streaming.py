"""Streaming lip-sync: live audio streams share each generator batch.

Every other entry point takes a finished recording.  Here audio arrives in chunks (`feed`), for many streams at once, and frames
leave as soon as the audio that determines them is there:

    streams = LipsyncStreams(model, batch_size=128, sink=deliver)
    streams.open(key, frames, boxes)          # uint8 [H,W,3] frames (cycled as inference.py does), one box per frame
    streams.feed(key, samples)                # float32 16 kHz samples, any chunk size
    streams.step()                            # per tick: new spectrogram columns, ready rows launched, finished frames delivered
    streams.close(key)                        # end of audio: the rows that depend on the end become ready
    streams.drain()                           # run and deliver everything that is ready or in flight

The contract: however a stream's audio of N samples is cut into `feed` calls and interleaved with other streams, the rows it
runs are exactly `multiclip.rows_inference(1 + N//200, len(frames), boxes, fps, static)`, in order, on a spectrogram that
equals `audio.melspectrogram_device(whole audio)` bit for bit.

The spectrogram is streamable exactly: column t reads samples [t*200 - 401, t*200 + 400), so it is FINAL once
t*200 + 400 <= the samples fed (the reflect padding only touches the two ends; the start is known, the end comes with `close`).
Per `step` the host stages, in ONE pinned buffer, the new samples of every stream plus the at most 801 earlier ones its next
columns read (it keeps that tail and nothing older), and ONE w2l_mel_stream_cols launch (csrc/audio_mel.hip) computes the newly
final columns of all streams into their windows.  Row i of an open stream is ready once the columns through start_i + 15 are
final.  Ready rows are taken in stream-open order, each stream's in row order, and packed by `multiclip.BatchRunner` into shared
batches on `depth` lanes: a full `batch_size` launches at once, the remainder with `flush=True` or in `drain`, padded to the next
of BUCKETS that is <= batch_size (else batch_size) by repeating the last row into a scratch frame - so the model holds a handful
of plans per lane however the ticks fall, each with committed launch configurations.  The batching is a deterministic function of
the call sequence.

Memory per stream does not grow with its duration: a spectrogram window of `mel_window` columns on the device.  When it is full
the stream continues in a FRESH window that starts with the at most 16 columns still needed; batches in flight keep the old one
alive (the runner's `keep=`), and no column is ever moved or overwritten under a batch that may read it.

`python -m wav2lip_amd.streaming --checkpoint_path C --face F0 --audio A0 --face F1 --audio A1 ... --outdir D` feeds every audio
file in `--chunk_ms` slices round-robin, steps after each round and writes one AVI per stream.
"""
import collections
import os

import numpy as np

from .inference import LIPSYNC_DEPTH, mel_step_size, validate_boxes
from .multiclip import BatchRunner, _align

HOP, NFFT = 200, 800                  # hparams.py: hop_size, n_fft (the kernels are specialised to them)
BUCKETS = (8, 16, 32, 64, 128)        # batch sizes of plan_configs.json's table a ragged batch is padded to
MIN_SAMPLES = NFFT // 2 + 1           # one reflection needs 401 samples (w2l_melspectrogram's own limit)
MIN_WINDOW = 64                       # columns: 16 carried over + room to go on
MAX_COLS_PER_LAUNCH = 1 << 20         # w2l_mel_stream_cols' limit

# numpy mirrors of w2l_mel_stream (48 bytes) and w2l_mel_col (16 bytes); the ctypes mirrors are _lib.MelStream / _lib.MelCol
MEL_STREAM = np.dtype([("samples", "<u8"), ("first", "<i8"), ("total", "<i8"), ("window", "<u8"), ("held", "<i4"), ("cap", "<i4"),
                       ("col0", "<i8")])
MEL_COL = np.dtype([("stream", "<i4"), ("rsv", "<i4"), ("col", "<i8")])


def final_columns(n, closed=False):
    """number of spectrogram columns that are final after n samples: all 1 + n//200 of a closed stream; on an open one the
    columns t with t*200 + 400 <= n - and column 0 needs sample 400 (the reflection of -400), hence 401 samples"""
    if closed:
        return 1 + n // HOP
    return 0 if n < MIN_SAMPLES else (n - NFFT // 2) // HOP + 1


def first_sample_needed(col):
    """the earliest sample any column >= col reads (window start, minus one for the pre-emphasis)"""
    return max(0, col * HOP - NFFT // 2 - 1)


def column_sample_range(col, total=-1):
    """[lo, hi] of the samples column `col` reads, reflections and the pre-emphasis predecessor included; total: the signal's
    length when it is known (closed stream), else -1"""
    lo, hi = col * HOP - NFFT // 2, col * HOP + NFFT // 2 - 1
    if lo < 0:
        lo, hi = 0, max(hi, -lo)
    if total >= 0 and hi >= total:
        lo, hi = min(lo, 2 * (total - 1) - hi), total - 1
    return max(0, lo - 1), hi


def row_start(i, fps):
    """inference.py:231-236: first column of chunk i (double multiply + truncation, as mel_chunk_starts)"""
    return int(i * (80. / fps))


def bucket(n, batch_size):
    """the size a ragged batch of n rows launches at"""
    for b in BUCKETS:
        if n <= b <= batch_size:
            return b
    return batch_size


class StreamState:
    """host bookkeeping of one stream, no device in it: samples held, columns done, the window's position, rows emitted"""

    def __init__(self, key, frames, boxes, static, fps, cap):
        self.key, self.frames, self.boxes, self.static, self.fps, self.cap = key, frames, boxes, bool(static), float(fps), int(cap)
        self.n_fed, self.closed = 0, False
        self.held, self.held_first, self.chunks = np.empty(0, np.float32), 0, []
        self.cols_done, self.col0, self.window = 0, 0, None
        self.next_row, self.rows_done, self.n_rows, self.delivered = 0, False, None, 0

    # ---- audio
    def feed(self, samples):
        if self.closed:
            raise ValueError("stream %r is closed" % (self.key,))
        x = np.ascontiguousarray(samples, dtype=np.float32)
        if x.ndim != 1:
            raise ValueError("feed: 1-D samples expected, got shape %s" % (x.shape,))
        if x.size:
            self.chunks.append(x.copy())
            self.n_fed += x.size

    def samples(self):
        """the held samples as one array (absolute index of [0]: held_first)"""
        if self.chunks:
            self.held = np.concatenate([self.held] + self.chunks)
            self.chunks = []
        return self.held

    # ---- columns
    def target(self):
        return final_columns(self.n_fed, self.closed)

    def plan(self):
        """what the next launch computes for this stream: None, or (roll, first column, count).  roll: None, or the absolute
        column a fresh window starts at because the columns wanted do not fit behind the ones done"""
        target = self.target()
        if target <= self.cols_done:
            return None
        roll, col0 = None, self.col0
        if target > col0 + self.cap:
            # keep what a row not yet emitted may read: from the next row's start, and the 16 columns the tail window of
            # mel_chunk_starts covers if the stream closed right now
            keep_from = max(0, min(row_start(self.next_row, self.fps), self.cols_done - mel_step_size))
            if keep_from > col0:
                roll = col0 = keep_from
        count = min(target, col0 + self.cap) - self.cols_done
        assert count > 0, "the spectrogram window cannot advance"
        return roll, self.cols_done, count

    def commit(self, count):
        self.cols_done += count
        x = self.samples()
        lo = first_sample_needed(self.cols_done)
        if self.closed:
            # every column done: no sample is needed again; else the reflected end reads back to n - 402
            lo = self.n_fed if self.cols_done == self.target() else min(lo, max(0, self.n_fed - NFFT // 2 - 2))
        if lo > self.held_first:
            self.held = x[lo - self.held_first:].copy()
            self.held_first = lo

    # ---- rows
    def take_rows(self):
        """rows that became ready, in order: (row index, frame index, box, absolute start column)"""
        out = []
        while not self.rows_done:
            s = row_start(self.next_row, self.fps)
            if s + mel_step_size <= self.cols_done:
                pass
            elif self.closed and self.cols_done == self.target():
                s = self.cols_done - mel_step_size            # the tail window, re-anchored at the end (inference.py:237-239)
                self.rows_done, self.n_rows = True, self.next_row + 1
            else:
                break
            fi = 0 if self.static else self.next_row % len(self.frames)
            out.append((self.next_row, fi, self.boxes[fi], s))
            self.next_row += 1
        return out

    def finished(self):
        return self.rows_done and self.delivered == self.n_rows


class DeviceMel:
    """the device side of the incremental spectrogram: windows, and one staged copy + one w2l_mel_stream_cols launch per call"""

    def __init__(self, device):
        import torch
        from . import _lib, audio
        self.torch, self.device = torch, device
        self.lib, self.ctx = _lib.load(), audio._context(device)

    def new_window(self, cap):
        return self.torch.zeros((80, cap), dtype=self.torch.float32, device=self.device)

    def carry(self, new, old, first, count):
        """columns [first, first + count) of `old` to the front of `new` (a fresh tensor: nothing reads it yet)"""
        new[:, :count].copy_(old[:, first:first + count])

    @staticmethod
    def window_bytes(window):
        return window.numel() * window.element_size()

    def compute(self, items):
        """items: (samples float32 array, absolute index of samples[0], total or -1, window, cap, col0, first column, count)"""
        from . import _lib
        from ._lib import check, ptr
        torch = self.torch
        ncols = sum(it[7] for it in items)
        off = _align(len(items) * MEL_STREAM.itemsize)
        col_off = off
        off = _align(off + ncols * MEL_COL.itemsize)
        at = []
        for it in items:
            at.append(off)
            off = _align(off + it[0].nbytes)
        host = torch.empty(off, dtype=torch.uint8, pin_memory=True)
        dev = torch.empty(off, dtype=torch.uint8, device=self.device)
        stage = host.numpy()
        st = stage[:len(items) * MEL_STREAM.itemsize].view(MEL_STREAM)
        ct = stage[col_off:col_off + ncols * MEL_COL.itemsize].view(MEL_COL)
        c = 0
        for k, (x, first, total, window, cap, col0, lo, count) in enumerate(items):
            stage[at[k]:at[k] + x.nbytes] = x.view(np.uint8)
            st[k] = (dev.data_ptr() + at[k], first, total, window.data_ptr(), x.size, cap, col0)
            ct["stream"][c:c + count] = k
            ct["rsv"][c:c + count] = 0
            ct["col"][c:c + count] = np.arange(lo, lo + count)
            c += count
        dev.copy_(host, non_blocking=True)
        with torch.cuda.device(self.device):
            for lo in range(0, ncols, MAX_COLS_PER_LAUNCH):
                n = min(MAX_COLS_PER_LAUNCH, ncols - lo)
                check(self.lib.w2l_mel_stream_cols(self.ctx, _lib.current_stream(), ptr(dev), len(items),
                                                   dev.data_ptr() + col_off + lo * MEL_COL.itemsize, n), "mel_stream_cols")


def check_coverage(x_first, x_size, total, lo, count, key=None):
    """the held samples [x_first, x_first + x_size) cover what columns [lo, lo + count) read; the kernel would clamp, and give
    wrong numbers - so this is checked before every launch.  The first and the last column bound the rest: a column's range
    moves up with the column, and on a closed stream the last column reflects furthest back from the end."""
    ranges = [column_sample_range(col, total) for col in {lo, lo + count - 1}]
    a, b = min(r[0] for r in ranges), max(r[1] for r in ranges)
    if a < x_first or b >= x_first + x_size:
        raise RuntimeError("stream %r: columns [%d, %d) read samples [%d, %d], held are [%d, %d)"
                           % (key, lo, lo + count, a, b, x_first, x_first + x_size))


def advance_columns(mel, states):
    """one staged copy + one launch on `mel` (a DeviceMel): the final columns every StreamState of `states` has window room
    for, rolling a full window over into a fresh one first; False when no stream had any"""
    items, done = [], []
    for st in states:
        p = st.plan()
        if p is None:
            continue
        roll, lo, count = p
        if roll is not None:
            fresh = mel.new_window(st.cap)
            if st.cols_done > roll:
                mel.carry(fresh, st.window, roll - st.col0, st.cols_done - roll)
            st.window, st.col0 = fresh, roll
        elif st.window is None:
            st.window = mel.new_window(st.cap)
        x = st.samples()
        total = st.n_fed if st.closed else -1
        check_coverage(st.held_first, x.size, total, lo, count, st.key)
        items.append((x, st.held_first, total, st.window, st.cap, st.col0, lo, count))
        done.append((st, count))
    if items:
        mel.compute(items)
        for st, count in done:
            st.commit(count)
    return bool(items)


class LipsyncStreams:
    """many live audio streams through one generator in shared batches (module docstring).  `sink(key, frame_u8)` receives every
    stream's frames in row order, then `sink(key, None)`; without a sink the frames are collected in `self.frames[key]` (which
    `drain` returns).  `on_batch(rows)` receives each launched batch's [(key, row index)] including the padding rows."""

    def __init__(self, model, batch_size=128, depth=None, precision="f32", fps=25., sink=None, on_batch=None, mel_window=1024):
        from .models.wav2lip import check_precision
        self.precision = check_precision(precision)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        if mel_window < MIN_WINDOW:
            raise ValueError("mel_window must be at least %d columns" % MIN_WINDOW)
        self.model, self.batch_size, self.depth, self.fps = model, int(batch_size), depth or LIPSYNC_DEPTH, float(fps)
        self.mel_window, self.on_batch = int(mel_window), on_batch
        self.frames = None
        if sink is None:
            self.frames = {}

            def sink(key, frame):
                lst = self.frames.setdefault(key, [])
                if frame is not None:
                    lst.append(frame)
        self.sink = sink
        self._streams = collections.OrderedDict()       # open order
        self._ready = collections.deque()                # (stream, row, frame index, box, (window, cap, relative start))
        self._pending = collections.deque()              # (ticket, [(stream, row)]) of the batches in flight, oldest first
        self._runner = self._mel = None
        self.launches = 0                                # w2l_mel_stream_cols staging copies + launches so far

    # ---- the stream's life
    def open(self, key, frames, boxes, static=False, fps=None):
        if key in self._streams:
            raise ValueError("stream %r is already open" % (key,))
        frames = list(frames)
        if not frames:
            raise ValueError("stream %r: no frames" % (key,))
        checked = []
        for f, b in zip(frames[:1] if static else frames, boxes):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("stream %r: frames must be uint8 [H,W,3] arrays" % (key,))
            try:
                checked.append(validate_boxes([b], f.shape[0], f.shape[1])[0])
            except ValueError as e:
                raise ValueError("stream %r: %s" % (key, e)) from None
        if len(checked) != (1 if static else len(frames)):
            raise ValueError("stream %r: one box per frame" % (key,))
        self._streams[key] = StreamState(key, frames, checked, static, self.fps if fps is None else fps, self.mel_window)

    def _get(self, key):
        try:
            return self._streams[key]
        except KeyError:
            raise KeyError("no open stream %r" % (key,)) from None

    def feed(self, key, samples):
        self._get(key).feed(samples)

    def close(self, key):
        st = self._get(key)
        if st.closed:
            raise ValueError("stream %r is closed" % (key,))
        n = st.n_fed
        if n < MIN_SAMPLES or final_columns(n, True) < mel_step_size:
            del self._streams[key]
            if n < MIN_SAMPLES:
                raise ValueError("stream %r: %d samples; the spectrogram's reflect padding needs more than %d" % (key, n, NFFT // 2))
            # lipsync() on such audio fails in w2l_mel_gather (T >= 16): the same exception type, at close
            raise RuntimeError("stream %r: %d samples give %d mel columns; the generator needs a window of %d"
                               % (key, n, final_columns(n, True), mel_step_size))
        st.closed = True

    # ---- the tick
    def _backend(self):
        if self._runner is None:
            self._runner = BatchRunner(self.model, self.batch_size, self.depth, self.precision)
            self._mel = DeviceMel(self._runner.device)

    def _columns_round(self):
        more = advance_columns(self._mel, self._streams.values())
        self.launches += more
        return more

    def step(self, flush=False):
        """compute the newly final columns (one launch for all streams; more only while a stream's backlog exceeds its window),
        launch the full batches of ready rows - with `flush` the remainder too - and deliver the batches that have finished"""
        self._backend()
        while True:
            more = self._columns_round()
            for st in self._streams.values():
                for row, fi, box, s in st.take_rows():
                    self._ready.append((st, row, fi, box, (st.window, st.cap, s - st.col0)))
            self._launch(False)
            if not more:
                break
        if flush:
            self._launch(True)
        while self._pending and self._runner.ready(self._pending[0][0]):
            self._collect()

    def _launch(self, flush):
        bs = self.batch_size
        while len(self._ready) >= bs or (flush and self._ready):
            rows = [self._ready.popleft() for _ in range(min(bs, len(self._ready)))]
            n = len(rows)
            size = bs if n == bs else bucket(n, bs)
            ticket = self._runner.submit([(st, fi, box, mel) for st, _, fi, box, mel in rows], pad_to=size)
            owners = [(st, row) for st, row, _, _, _ in rows]
            if self.on_batch is not None:
                self.on_batch([(st.key, row) for st, row in owners] + [(owners[-1][0].key, owners[-1][1])] * (size - n))
            self._pending.append((ticket, owners))
            if len(self._pending) >= self.depth:
                self._collect()

    def _collect(self):
        item, owners = self._pending.popleft()
        for (st, _), frame in zip(owners, self._runner.result(item)):
            self.sink(st.key, frame)
            st.delivered += 1
            if st.finished():
                if self._streams.get(st.key) is st:
                    del self._streams[st.key]
                st.frames = st.window = None
                self.sink(st.key, None)

    def drain(self):
        """close nothing; run and deliver everything that is ready or in flight"""
        self.step(flush=True)
        while self._pending:
            self._collect()
        return self.frames

    def device_bytes(self, key=None):
        """device memory held per stream between ticks: its spectrogram window (the staging of a tick is transient)"""
        sts = self._streams.values() if key is None else [self._get(key)]
        return sum(DeviceMel.window_bytes(st.window) for st in sts if st.window is not None)


# ---------------------------------------------------------------- command line
def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="Lip-sync several faces to audio that arrives in chunks, in shared generator batches")
    p.add_argument('--checkpoint_path', type=str, required=True, help='Name of saved checkpoint to load weights from')
    p.add_argument('--face', type=str, action='append', required=True, help='Video/image of one stream (repeat, one per --audio)')
    p.add_argument('--audio', type=str, action='append', required=True, help='16-bit WAV of one stream (repeat, one per --face)')
    p.add_argument('--outdir', type=str, default='results', help='Stream k is written to <outdir>/<k>.avi')
    p.add_argument('--chunk_ms', type=float, default=40., help='Milliseconds of audio fed to every stream per tick')
    p.add_argument('--static', type=bool, default=False, help='If True, then use only first video frame for inference')
    p.add_argument('--fps', type=float, default=25., help='Can be specified only if input is a static image (default: 25)')
    p.add_argument('--pads', nargs='+', type=int, default=[0, 10, 0, 0], help='Padding (top, bottom, left, right)')
    p.add_argument('--face_det_batch_size', type=int, default=16, help='Batch size for face detection')
    p.add_argument('--wav2lip_batch_size', type=int, default=128, help='Batch size for Wav2Lip model(s)')
    p.add_argument('--resize_factor', default=1, type=int, help='Reduce the resolution by this factor')
    p.add_argument('--crop', nargs='+', type=int, default=[0, -1, 0, -1], help='Crop video to a smaller region (top, bottom, left, right)')
    p.add_argument('--box', nargs='+', type=int, default=[-1, -1, -1, -1],
                   help='Constant bounding box for the face (top, bottom, left, right) instead of face detection')
    p.add_argument('--rotate', default=False, action='store_true', help='Rotate the video right by 90deg')
    p.add_argument('--nosmooth', default=False, action='store_true', help='Prevent smoothing face detections over a short temporal window')
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'], help='Generator arithmetic')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'], help='Face detector arithmetic')
    from .inference import add_det_scale_flag
    add_det_scale_flag(p)
    return p


def main(argv=None):
    """feed every `--audio` in `--chunk_ms` slices round-robin to its `--face`, step after each round, write <outdir>/<k>.avi as
    each stream ends; returns the written paths in stream order"""
    import copy

    import torch

    from . import audio, inference
    a = build_parser().parse_args(argv)
    if len(a.face) != len(a.audio):
        raise ValueError("%d --face for %d --audio: pass them in pairs" % (len(a.face), len(a.audio)))
    dev = torch.device("cuda", torch.cuda.current_device())
    jobs = []
    for k, (face, wav_path) in enumerate(zip(a.face, a.audio)):
        one = copy.copy(a)
        one.face = face
        if os.path.isfile(face) and inference.is_image_path(face):
            one.static = True
        frames, fps = inference.read_frames(one)
        if not wav_path.endswith('.wav'):
            raise ValueError("--audio %s: pass a .wav" % wav_path)
        if a.box[0] == -1:
            det = inference.face_detect(frames if not one.static else [frames[0]], pads=a.pads, nosmooth=a.nosmooth,
                                        batch_size=a.face_det_batch_size, precision=inference.CLI_PRECISION[a.face_det_precision],
                                        det_scale=a.face_det_scale)
            boxes = [c for _, c in det]
        else:
            boxes = [tuple(a.box)] * len(frames)
        jobs.append(dict(key=k, frames=frames, fps=fps, boxes=boxes, static=one.static, wav=audio.load_wav(wav_path, 16000),
                         audio=wav_path, out=os.path.join(a.outdir, "%d.avi" % k), pos=0))
    os.makedirs(a.outdir, exist_ok=True)
    model = inference.load_model(a.checkpoint_path, dev)
    got = {j["key"]: [] for j in jobs}

    def sink(key, frame):
        if frame is not None:
            got[key].append(frame)
            return
        j = jobs[key]
        inference.write_result(j["out"], got.pop(key), j["fps"], j["audio"])

    streams = LipsyncStreams(model, batch_size=a.wav2lip_batch_size, precision=inference.CLI_PRECISION[a.precision], sink=sink)
    for j in jobs:
        streams.open(j["key"], j["frames"], j["boxes"], static=j["static"], fps=j["fps"])
    chunk = max(1, int(round(16000 * a.chunk_ms / 1000.)))
    live = list(jobs)
    while live:
        for j in live:
            streams.feed(j["key"], j["wav"][j["pos"]:j["pos"] + chunk])
            j["pos"] += chunk
            if j["pos"] >= len(j["wav"]):
                streams.close(j["key"])
        live = [j for j in live if j["pos"] < len(j["wav"])]
        streams.step()
    streams.drain()
    return [j["out"] for j in jobs]


if __name__ == '__main__':
    main()
