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
Per `step` the host stages, in ONE pinned buffer (every staging buffer of this module is laid out by staging.py), the new
samples of every stream plus the at most 801 earlier ones its next columns read (it keeps that tail and nothing older), and
ONE w2l_mel_stream_cols launch (csrc/audio_mel.hip) computes the newly final columns of all streams into their windows.  Row i of an open stream is ready once the columns through start_i + 15 are
final.  Ready rows are taken in stream-open order, each stream's in row order, and packed by `multiclip.BatchRunner` into shared
batches on `depth` lanes: a full `batch_size` launches at once, the remainder with `flush=True` or in `drain`, padded to the next
of BUCKETS that is <= batch_size (else batch_size) by repeating the last row into a scratch frame - so the model holds a handful
of plans per lane however the ticks fall, each with committed launch configurations.  The batching is a deterministic function of
the call sequence.

Memory per stream does not grow with its duration: a spectrogram window of `mel_window` columns on the device.  When it is full
the stream continues in a FRESH window that starts with the at most 16 columns still needed; batches in flight keep the old one
alive (the runner's `keep=`), and no column is ever moved or overwritten under a batch that may read it.

Audio at its own rate.  No live source delivers float32 mono at 16 kHz: microphones, WebRTC and capture cards
give 48 kHz or 44.1 kHz int16, often stereo.

    streams.open(key, frames, boxes, sample_rate=48000)       # `open_live(key, sample_rate=...)` likewise
    streams.feed(key, pcm)                    # what a WAV of that rate decodes to: int16 / int32 / uint8 / float32 / float64,
                                              # 1-D or [n, channels]; converted and mixed down as `audio.load_wav` does

The contract: a stream opened at rate R and fed N source samples in all, however they are cut and interleaved, has a spectrogram
that equals `audio.melspectrogram_device(audio.resample(whole, R, 16000))` bit for bit, and runs exactly the rows
`multiclip.rows_inference(1 + M // 200, ...)` with M = ceil(N * 16000 / R), in order; the batching stays a deterministic function
of the call sequence.  The conversion is `audio.resample`'s (librosa.load's resampy 'kaiser_best') and can keep that contract
because its filter is finite: with ratio = 16000 / R, index_step = int(min(1, ratio) * 512) and K = 32769 // index_step (192
source samples at 48 kHz, 177 at 44.1 kHz, 64 when the rate goes up) the output sample t, whose time register has the integer
part n_t, reads the source samples n_t - K + 1 .. n_t + K: with m samples fed it is FINAL once n_t + K <= m - 1.  Per `step` ONE
staged copy (the new source samples of every such stream plus the at most K + 1 earlier ones the left wings read) and ONE
w2l_resample_stream launch (csrc/audio_mel.hip) compute the newly final 16 kHz samples of all streams, whatever their rates, into
per-stream device buffers of `resample_buffer` samples; w2l_mel_stream_cols reads them where they lie, with the count of final
samples in the place of the samples fed.  The time register is continued by sequential float64 addition from tick to tick, as the
reference accumulates it.  A full buffer continues in a fresh one whose head - the at most 801 samples a column not yet done
reads - is copied in the same launch.  `close` applies its length checks to M.  A stream at 16000 Hz is what it always was: the
same launches, float32 1-D input only.  `launches` counts the spectrogram launches, `resample_launches` these.

Live video.  A stream whose camera frames arrive with its audio has neither frames nor boxes to open with:

    streams = LipsyncStreams(model, sink=deliver, detector=face_detection.FaceAlignment(...), pads=(0, 10, 0, 0), smooth_T=5)
    streams.open_live(key)                    # no frames, no boxes; cycle=False: the rows end with the video
    streams.feed_frames(key, frames)          # uint8 [H,W,3] BGR host arrays, or one uint8 device tensor [n,H,W,3]
    streams.close_video(key)                  # end of video; `close(key)` still ends the audio

The contract, next to the one above: however a live stream's audio and frames are cut into `feed` / `feed_frames` calls and
interleaved with other streams, with F the frames it was fed the rows it runs are exactly
`multiclip.rows_inference(n_mel, len(F), boxes, fps)` - or, with cycle=False, their first `min(len(rows), len(F))` - where `boxes`
is the finish of `face_detect(F, detector, pads, nosmooth=(smooth_T == 0))` (pads, clipping, smoothing, "no face") on the rects
the detector gives IN WHOLE BATCHES of `face_det_batch_size` frames, the last batch padded with its last frame.  A rect from a
whole batch does not depend on which frames fill the batch; `face_detect` itself ends a video in a ragged batch, and a
detector's launches are a function of the batch size.  With the fp32 detector the rects of a ragged batch have been equal on
every clip tried, so the boxes are `face_detect`'s as it stands; with `precision="bf16"` another split-K factor sums in another
order and a rect of the ragged batch does come out different now and then (4 boxes of a 52-frame clip) - there
the boxes are those of `face_detect` run in whole batches.  The finish is exact because `get_smoothened_boxes` looks forward: box i is final once frame i + smooth_T - 1 has
been detected, and the last boxes once the video is closed (face_detection/live.py).
Per `step` the frames fed since the last one go up in ONE pinned buffer, through detector batches of exactly
`face_det_batch_size`, and ONE w2l_face_boxes_stream launch (csrc/detect.hip) finishes the boxes of all streams; the NEXT `step`
first waits for that launch's event (it never polls, so the batching stays a function of the call sequence).  Row i is ready
when its spectrogram window is final and frame i % n_frames is there with a final box: boxes lag smooth_T - 1 frames plus one
tick.  The uploaded frames stay on the device and the generator reads them there.  By default (the reference's rule) a frame
without a face ends its stream only: the rows already taken are delivered, `sink(key, None)` follows and `errors[key]` says why.
A stream is gone once its last row is delivered; `feed` / `feed_frames` on it then raise KeyError.

Frames without a face (opt-in, not the reference's behaviour).  `LipsyncStreams(..., no_face_hold=G)` with G in
0..250 keeps such a stream alive: the frame keeps the last detected rect for up to G frames (no look-ahead) and is a gap frame
beyond that, and every run of boxed frames is padded, clipped and smoothed as a video of its own
(`face_detection.many.host_boxes_runs` on the finished video, whatever the cut; ONE w2l_face_boxes_stream_runs launch per tick in
the place of w2l_face_boxes_stream).  A gap frame's row becomes ready exactly when a boxed one would, takes no batch row, and is
delivered unchanged - the input frame's bytes - by the same `sink` in its place in the row order; `errors` stays empty for it.
Readiness of the other rows, bucketing and `on_batch` see boxed rows only, so the batching stays a function of the call sequence.
`open(key, frames, boxes)` then accepts None among `boxes` with the same meaning.

`python -m wav2lip_amd.streaming --checkpoint_path C --face F0 --audio A0 --face F1 --audio A1 ... --outdir D` feeds every audio
file in `--chunk_ms` slices round-robin, steps after each round and writes one AVI per stream; with `--live_video` every video is
fed frame by frame as its audio goes by and `face_detect` is never called; with `--native_rate` every WAV is fed at the file's
own rate and sample format instead of being converted up front.
"""
import collections
import os

import numpy as np

from ._lib import MEL_COL, MEL_STREAM, RESAMPLE_BLOCKS, RESAMPLE_STREAM, TRACK_SEGMENT
from .inference import LIPSYNC_DEPTH, mel_step_size, validate_boxes
from .multiclip import BatchRunner
from .staging import ADDRESS, Staging

HOP, NFFT = 200, 800                  # hparams.py: hop_size, n_fft (the kernels are specialised to them)
BUCKETS = (8, 16, 32, 64, 128)        # batch sizes of plan_configs.json's table a ragged batch is padded to
MIN_SAMPLES = NFFT // 2 + 1           # one reflection needs 401 samples (w2l_melspectrogram's own limit)
MIN_WINDOW = 64                       # columns: 16 carried over + room to go on
MAX_COLS_PER_LAUNCH = 1 << 20         # w2l_mel_stream_cols' limit

RATE16 = 16000                        # hparams.py: sample_rate, the rate the spectrogram is specialised to
RESAMPLE_TABLE, RESAMPLE_NWIN = 512, 64 * 512 + 1         # resampy's kaiser_best: table samples per zero crossing, half window
RESAMPLE_BLOCK = 128                  # outputs per block entry of w2l_resample_stream (one thread each)
MAX_BLOCKS_PER_LAUNCH = 1 << 20       # w2l_resample_stream's limit
MIN_BUFFER16 = 2048                   # 16 kHz samples: the at most 801 the spectrogram still reads + room to go on


def resample_params(rate):
    """(ratio, increment of the time register, scale, index_step, K) of resampy's kaiser_best from `rate` to 16 kHz; K is how
    many source samples each wing of the filter reaches.  ValueError for a rate that is no positive integer or whose table step
    would be 0 (above 8 192 000 Hz)"""
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or rate < 1:
        raise ValueError("sample_rate must be a positive integer, got %r" % (rate,))
    ratio = float(RATE16) / int(rate)
    scale = min(1.0, ratio)
    index_step = int(scale * RESAMPLE_TABLE)
    if index_step < 1:
        raise ValueError("sample_rate %d: the interpolation table has no step that small (at most %d Hz)" % (rate, RATE16 * RESAMPLE_TABLE))
    return ratio, 1.0 / ratio, scale, index_step, RESAMPLE_NWIN // index_step


def resample_sample_range(tr, K, total=-1):
    """[lo, hi] of the source samples the output with time register `tr` reads: its left wing x[n], x[n-1], ... and its right
    wing x[n+1], ..., K samples each at the most, cut by the start and - total: the signal's length once known, else -1 - the end"""
    n = int(tr)
    return max(0, n - K + 1), (n + K if total < 0 else max(n, min(n + K, total - 1)))


def native_samples(samples):
    """what `audio.load_wav` makes of decoded PCM before it resamples, with its numpy expressions: int16 / int32 / uint8 /
    float32 / float64, 1-D or [n, channels] -> float32 mono.  Both steps are sample-wise, so they do not depend on the cut."""
    from . import audio
    data = np.asarray(samples)
    if data.ndim not in (1, 2) or data.dtype not in (np.int16, np.int32, np.uint8, np.float32, np.float64):
        raise ValueError("feed: int16, int32, uint8, float32 or float64 samples, 1-D or [n, channels], expected; got %s %s"
                         % (data.dtype, data.shape))
    x = audio._pcm_to_float32(data)
    if x.ndim > 1:
        x = x.T.mean(axis=0)
    return np.ascontiguousarray(x, dtype=np.float32)


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


class HeldSamples:
    """samples that arrive in chunks and leave from the front: chunks appended, concatenated on demand, `held_first` the
    absolute index of `samples()[0]`"""

    def __init__(self):
        self.held, self.held_first, self.chunks = np.empty(0, np.float32), 0, []

    def samples(self):
        """the held samples as one array (absolute index of [0]: held_first)"""
        if self.chunks:
            self.held = np.concatenate([self.held] + self.chunks)
            self.chunks = []
        return self.held

    def drop_below(self, lo):
        """let go of the samples before the absolute index `lo`"""
        x = self.samples()
        if lo > self.held_first:
            self.held = x[lo - self.held_first:].copy()
            self.held_first = lo


class ResampleState(HeldSamples):
    """host bookkeeping of one stream's conversion to 16 kHz, no device in it: the source samples a later
    output's left wing reads, the running time register, the count of final 16 kHz samples and where they lie"""

    def __init__(self, key, rate, cap16):
        self.key, self.rate, self.cap16 = key, int(rate), int(cap16)
        self.ratio, self.inc, self.scale, self.index_step, self.K = resample_params(rate)
        self.n_src, self.closed = 0, False
        HeldSamples.__init__(self)            # the source samples a later output's left wing reads
        self.n16, self.tr_next = 0, 0.0       # final 16 kHz samples computed; the time register of the next one
        self.n_res = self.total16 = None      # after close: resampy's int(N * ratio), librosa's ceil(N * ratio)
        self.buf, self.buf_first = None, 0    # the device buffer that holds the 16 kHz samples [buf_first, n16)
        self.need16 = 0                       # the first 16 kHz sample a spectrogram column not yet done reads

    def feed(self, x):
        if x.size:
            self.chunks.append(x)
            self.n_src += x.size

    def close(self):
        self.closed = True
        self.n_res, self.total16 = int(self.n_src * self.ratio), int(np.ceil(self.n_src * self.ratio))

    def registers(self, count):
        """the time registers of the next `count` outputs: the running one continued by sequential float64 addition (cumsum),
        as the reference accumulates them - never t * increment"""
        inc = np.full(count, self.inc, dtype=np.float64)
        inc[0] = self.tr_next
        return np.cumsum(inc)

    def new_final(self, at_most):
        """(how many of the next `at_most` outputs are final, their time registers).  Output t with n = int(register) reads up
        to source sample n + K: final once n + K <= n_src - 1, i.e. register < n_src - K; all of them once the stream is closed"""
        if self.closed:
            c = min(at_most, self.total16 - self.n16)
            return c, (self.registers(c) if c else None)
        limit = self.n_src - self.K
        est = min(at_most, int(max(0.0, limit - self.tr_next) * self.ratio) + 2)
        while limit > 0:
            tr = self.registers(est)
            c = int(np.searchsorted(tr, limit, "left"))
            if c < est or est == at_most:
                return c, tr[:c]
            est = min(at_most, 2 * est)
        return 0, None

    def plan(self):
        """what the next launch computes: None, or (roll, first output, count, time registers).  roll: None, or the absolute
        16 kHz sample a fresh buffer starts at because the outputs wanted do not fit behind the ones done"""
        c, tr = self.new_final(self.cap16)
        if c == 0:
            return None
        roll, first = None, self.buf_first
        if self.n16 + c > first + self.cap16 and self.need16 > first:
            roll = first = self.need16
        c = min(c, first + self.cap16 - self.n16)
        if c <= 0:
            return None                       # full of samples the spectrogram has yet to read
        return roll, self.n16, c, tr[:c]

    def commit(self, count, tr):
        self.n16 += count
        self.tr_next = float(tr[count - 1]) + self.inc
        self.drop_below(self.n_src if self.closed and self.n16 == self.total16 else max(0, int(self.tr_next) - self.K))


class Resident:
    """samples that already lie on the device: `size` float32 values from element `offset` of `buffer` (a stream's 16 kHz
    buffer).  `DeviceMel.compute` reads them where they lie and stages nothing: to `Staging.place` this is a device object."""

    def __init__(self, buffer, offset, size):
        self.buffer, self.offset, self.size, self.nbytes = buffer, int(offset), int(size), 4 * int(size)

    def data_ptr(self):
        return self.buffer.data_ptr() + 4 * self.offset


class StreamState(HeldSamples):
    """host bookkeeping of one stream, no device in it: samples held, columns done, the window's position, rows emitted.
    sample_rate other than 16000: the samples fed are converted on the device first (`rs`, a ResampleState with a buffer of
    `cap16` samples) and the spectrogram reads the 16 kHz samples there."""
    live = False

    def __init__(self, key, frames, boxes, static, fps, cap, sample_rate=RATE16, cap16=MIN_BUFFER16):
        self.key, self.frames, self.boxes, self.static, self.fps, self.cap = key, frames, boxes, bool(static), float(fps), int(cap)
        self.n_fed, self.closed = 0, False
        HeldSamples.__init__(self)            # the 16 kHz samples a column not yet done reads (none with `rs`: those lie on the device)
        self.cols_done, self.col0, self.window = 0, 0, None
        self.next_row, self.rows_done, self.n_rows, self.delivered = 0, False, None, 0
        self.rs = None if sample_rate == RATE16 else ResampleState(key, sample_rate, cap16)

    # ---- audio
    def feed(self, samples):
        if self.closed:
            raise ValueError("stream %r is closed" % (self.key,))
        if self.rs is not None:
            self.rs.feed(native_samples(samples))
            return
        x = np.ascontiguousarray(samples, dtype=np.float32)
        if x.ndim != 1:
            raise ValueError("feed: 1-D samples expected, got shape %s" % (x.shape,))
        if x.size:
            self.chunks.append(x.copy())
            self.n_fed += x.size

    def end_audio(self):
        """no more samples follow"""
        self.closed = True
        if self.rs is not None:
            self.rs.close()

    def mel_samples(self):
        """the 16 kHz samples the spectrogram can read so far"""
        return self.n_fed if self.rs is None else self.rs.n16

    def mel_closed(self):
        """closed for the spectrogram: the stream is closed and every 16 kHz sample of it is there"""
        return self.closed and (self.rs is None or self.rs.n16 == self.rs.total16)

    # ---- columns
    def target(self):
        return final_columns(self.mel_samples(), self.mel_closed())

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
        n = self.mel_samples()
        lo = first_sample_needed(self.cols_done)
        if self.mel_closed():
            # every column done: no sample is needed again; else the reflected end reads back to n - 402
            lo = n if self.cols_done == self.target() else min(lo, max(0, n - NFFT // 2 - 2))
        if self.rs is not None:
            self.rs.need16 = lo               # the samples stay where they are: a fresh 16 kHz buffer starts here
            return
        self.drop_below(lo)

    # ---- rows
    def take_rows(self):
        """rows that became ready, in order: (row index, frame index, box, absolute start column)"""
        out = []
        while not self.rows_done:
            s = row_start(self.next_row, self.fps)
            if s + mel_step_size <= self.cols_done:
                pass
            elif self.mel_closed() and self.cols_done == self.target():
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

    def locate(self, fi):
        """(the object whose `.frames` the runner reads frame fi from, its index there)"""
        return self, fi

    def release_delivered(self):
        """called after every delivered row; a live stream lets go of frames no later row reads"""


class FrameChunk:
    """the frames [first, first + n) of a live stream, resident on the device: what one tick uploaded for it (a view of the
    tick's staging buffer), or a tensor the caller fed.  `BatchRunner` reads `.frames` where it lies."""

    def __init__(self, key, first, frames):
        self.key, self.first, self.frames, self.n = key, int(first), frames, int(frames.shape[0])
        self.nbytes = self.n * int(frames.shape[1]) * int(frames.shape[2]) * 3


class LiveState(StreamState):
    """a stream whose video arrives with its audio (`open_live`): the frames fed since the last tick, the chunks resident on
    the device, the boxes that are final so far - still no device in it"""
    live = True

    def __init__(self, key, fps, cap, cycle, sample_rate=RATE16, cap16=MIN_BUFFER16):
        StreamState.__init__(self, key, None, [], False, fps, cap, sample_rate=sample_rate, cap16=cap16)
        self.cycle = bool(cycle)
        self.shape = None                     # (H, W): fixed by the first frame fed
        self.fresh, self.n_frames = [], 0     # host arrays / device tensors fed since the last tick; frames fed in all
        self.seen = 0                         # frames handed to the detector
        self.video_closed = self.close_sent = self.video_done = False      # close_video called / in a launch / its boxes final
        self.video = []                       # FrameChunks, in frame order
        self.error = None

    def feed_frames(self, frames):
        if self.video_closed:
            raise ValueError("stream %r: its video is closed" % (self.key,))
        if hasattr(frames, "data_ptr"):
            if str(frames.dtype) != "torch.uint8" or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("stream %r: a frame tensor must be uint8 [n,H,W,3], got %s %s"
                                 % (self.key, frames.dtype, tuple(frames.shape)))
            items, shapes = ([frames.contiguous()] if frames.shape[0] else []), [tuple(int(v) for v in frames.shape[1:3])]
        else:
            if isinstance(frames, np.ndarray) and frames.ndim == 3:
                frames = [frames]
            items = []
            for f in frames:
                if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                    raise ValueError("stream %r: frames must be uint8 [H,W,3] arrays" % (self.key,))
                items.append(np.ascontiguousarray(f).copy())
            shapes = [f.shape[:2] for f in items]
        for s in shapes:
            if min(s) < 1 or (self.shape or s) != s or s != shapes[0]:
                raise ValueError("stream %r: a frame of shape %s in a stream of %s frames" % (self.key, s, self.shape or shapes[0]))
        if items:
            self.shape = shapes[0]
            self.fresh += items
            self.n_frames += sum(int(f.shape[0]) if hasattr(f, "data_ptr") else 1 for f in items)

    def n_fresh(self):
        return self.n_frames - self.seen

    def plan(self):
        """`StreamState.plan`; but a window full of columns whose rows still wait for their frames can neither advance nor
        roll over: then the samples wait on the host until rows have been taken"""
        keep_from = max(0, min(row_start(self.next_row, self.fps), self.cols_done - mel_step_size))
        if self.target() > self.cols_done >= self.col0 + self.cap and keep_from <= self.col0:
            return None
        return StreamState.plan(self)

    def take_rows(self):
        """`StreamState.take_rows` with the second condition of a live row: frame i % n_frames is there with a final box.
        While the video is open that is frame i itself; once the closed video's boxes are all final the rows cycle over it, or
        with cycle=False end with it."""
        out = []
        while not self.rows_done:
            i = self.next_row
            if self.video_done and not self.cycle and i >= self.n_frames:
                self.rows_done, self.n_rows = True, i         # the prefix of the rows that the video covers
                break
            s, tail = row_start(i, self.fps), False
            if s + mel_step_size <= self.cols_done:
                pass
            elif self.mel_closed() and self.cols_done == self.target():
                s, tail = self.cols_done - mel_step_size, True
            else:
                break
            if self.video_done:
                fi = i % self.n_frames
            elif i < len(self.boxes):
                fi = i
            else:
                break
            if tail:
                self.rows_done, self.n_rows = True, i + 1
            out.append((i, fi, self.boxes[fi], s))
            self.next_row += 1
        return out

    def locate(self, fi):
        for ch in reversed(self.video):
            if ch.first <= fi:
                return ch, fi - ch.first
        raise RuntimeError("stream %r: frame %d is not resident" % (self.key, fi))

    def release_delivered(self):
        if not self.cycle:                    # row i reads frame i: a chunk whose rows are all delivered is read no more
            while self.video and self.delivered >= self.video[0].first + self.video[0].n:
                self.video.pop(0)


class DeviceBoxes:
    """the device side of live face detection: per call one staged copy, the detector batches, ONE w2l_face_boxes_stream launch
    (csrc/detect.hip) for every stream of the tick and one copy back"""

    def __init__(self, device, detector, pads, T, batch_size, hold=None, track=None):
        """hold: None, or the G of the pass-through rule: w2l_face_boxes_stream_runs finishes the boxes, with its own carry slots.
        track: None, or a FaceTrack: the batches leave candidates and ONE w2l_face_track_segments launch per tick, between
        detection and the finish, follows each stream's face on from the state in its slot of `track_state`"""
        import torch
        from . import _lib
        from .face_detection import live
        self.torch, self.device, self.lib, self.live = torch, device, _lib.load(), live
        self.detector, self.pads, self.T, self.B, self.hold = detector, pads, T, batch_size, hold
        slot = (live.CARRY_ROWS, 4) if hold is None else (live.RUNS_CARRY_INTS,)
        self.carry = torch.zeros((64,) + slot, dtype=torch.int32, device=device)
        self.track = track
        if track is not None:
            from .face_detection.track import STATE_INTS
            self.track_state = torch.zeros((64, STATE_INTS), dtype=torch.int32, device=device)

    def reserve(self, n_slots):
        """room for carry slots [0, n_slots); the table grows on the launches' stream, so in order with them"""
        old = self.carry.shape[0]

        def grown(table):
            new = self.torch.zeros((max(n_slots, 2 * old),) + tuple(table.shape[1:]), dtype=self.torch.int32, device=self.device)
            new[:old].copy_(table)
            return new

        if n_slots > old:
            self.carry = grown(self.carry)
            if self.track is not None:
                self.track_state = grown(self.track_state)

    def launch(self, items):
        """items: [(fresh, H, W, slot, seen, closed)] - `fresh` the stream's new frames in order (host arrays, device tensors
        [n,H,W,3]).  Returns a ticket; `ticket["chunks"][k]` are item k's new frames on the device, [(frame count, tensor)]:
        runs of host frames as views of the staging buffer, fed tensors as they are."""
        from ._lib import check, current_stream, ptr
        from .face_detection.many import BoxOut, detect_rows, track_rows
        torch, live, B, T = self.torch, self.live, self.B, self.T
        SEG = live.BOX_STREAM_SEGMENT
        # ---- rows: the items of one frame shape are one run of arena rows, padded to whole detector batches
        runs, n_new, groups = [], [], collections.OrderedDict()
        for k, (fresh, H, W, _, _, _) in enumerate(items):
            mine = []                                      # [host arrays] or a tensor, consecutive host frames joined
            for f in fresh:
                if hasattr(f, "data_ptr"):
                    mine.append(f)
                elif mine and isinstance(mine[-1], list):
                    mine[-1].append(f)
                else:
                    mine.append([f])
            runs.append(mine)
            n_new.append(sum(len(r) if isinstance(r, list) else int(r.shape[0]) for r in mine))
            if n_new[k]:
                groups.setdefault((H, W), []).append(k)
        row0, spans, total = {}, [], 0
        for (H, W), members in groups.items():
            first = total
            for k in members:
                row0[k] = total
                total += n_new[k]
            padded = first + (total - first + B - 1) // B * B
            spans.append((H, W, first, total, padded))
            total = padded
        # ---- one staging buffer: [address table][segment table][the frames that were host arrays]
        st = Staging(self.device)
        addresses, segments = st.table(ADDRESS, total), st.table(SEG, len(items))
        tracks = None if self.track is None else st.table(TRACK_SEGMENT, len(items))
        src = [[st.place(run) for run in mine] for mine in runs]
        st.allocate()
        addr, segs = st.view(addresses), st.view(segments)
        chunks, out0 = [], 0
        for k, (fresh, H, W, slot, seen, closed) in enumerate(items):
            fb, r, mine = H * W * 3, row0.get(k, 0), []
            for h in src[k]:
                n = h.nbytes // fb
                addr[r:r + n] = np.uint64(st.address(h)) + np.arange(n, dtype=np.uint64) * np.uint64(fb)
                mine.append((n, st.tensor(h).view(n, H, W, 3)))
                r += n
            chunks.append(mine)
            segs[k] = (row0.get(k, 0), n_new[k], H, W, slot, seen, int(bool(closed)), out0)
            if tracks is not None:
                st.view(tracks)[k] = (row0.get(k, 0), n_new[k], slot, seen)
            out0 += live.new_final_count(seen, n_new[k], closed, T)
        for H, W, first, end, padded in spans:
            addr[end:padded] = addr[end - 1]               # the last batch of a shape: its last address again, into scratch rows
        st.upload()
        arenas = detect_rows(self.detector, st.tensor(addresses), [(H, W, first, padded) for H, W, first, _, padded in spans], B,
                             max(total, 1), self.track)
        out = BoxOut(out0, len(items), self.hold is not None, self.track is not None, self.device)     # one copy back
        top, bottom, left, right = self.pads
        with torch.cuda.device(self.device):
            if self.track is not None:                   # every stream's face followed on from its slot: selection is causal, so
                track_rows(len(items), st.tensor(tracks), arenas, self.track, out.track_status,       # box i is still final once
                           state=self.track_state)                                                    # frame i + T - 1 is there
            if self.hold is None:
                check(self.lib.w2l_face_boxes_stream(current_stream(), len(items), st.host_address(segments), st.address(segments),
                                                     ptr(arenas.rects), ptr(arenas.flags), total, ptr(self.carry),
                                                     int(self.carry.shape[0]), top, bottom, left, right, T, out.ptr(out.boxes), out0,
                                                     out.ptr(out.status)), "face_boxes_stream")
            else:
                check(self.lib.w2l_face_boxes_stream_runs(current_stream(), len(items), st.host_address(segments), st.address(segments),
                                                          ptr(arenas.rects), ptr(arenas.flags), total, ptr(self.carry),
                                                          int(self.carry.shape[0]), top, bottom, left, right, T, self.hold,
                                                          out.ptr(out.boxes), out.ptr(out.valid), out0, out.ptr(out.status)),
                      "face_boxes_stream_runs")
        host_out = torch.empty(out.buffer.numel(), dtype=torch.int32, pin_memory=True)
        host_out.copy_(out.buffer, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        counts = [int(c) for c in np.diff(np.append(segs["out0"], out0))]
        # the arenas of a track are freed in stream order: nothing else holds them
        return dict(chunks=chunks, counts=counts, host_out=host_out, done=done, keep=(st.host, st.dev, arenas.rects, arenas.flags),
                    out=out)

    @staticmethod
    def collect(ticket):
        """wait for the launch's event; [(boxes int32 [count,4] of (y1, y2, x1, x2), (code, frame))] per item, with a hold
        [(boxes, (code, frame), valid int32 [count])]"""
        ticket["done"].synchronize()
        boxes, valid, status, _ = ticket["out"].split(ticket["host_out"].numpy(), of="stream")
        out, r = [], 0
        for k, c in enumerate(ticket["counts"]):
            item = (boxes[r:r + c].copy(), (int(status[k][0]), int(status[k][1])))
            out.append(item if valid is None else item + (valid[r:r + c].copy(),))
            r += c
        return out


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
        """items: (samples float32 array, absolute index of samples[0], total or -1, window, cap, col0, first column, count);
        samples may be a `Resident` instead: they lie on the device already and nothing is staged for them"""
        from . import _lib
        from ._lib import check, ptr
        torch = self.torch
        ncols = sum(it[7] for it in items)
        stage = Staging(self.device)
        streams, cols = stage.table(MEL_STREAM, len(items)), stage.table(MEL_COL, ncols)
        src = [stage.place(it[0]) for it in items]
        stage.allocate()
        st, ct = stage.view(streams), stage.view(cols)
        ct["rsv"] = 0
        col_stream, col_col, c = ct["stream"], ct["col"], 0
        for k, (x, first, total, window, cap, col0, lo, count) in enumerate(items):
            st[k] = (stage.address(src[k]), first, total, window.data_ptr(), x.size, cap, col0)
            col_stream[c:c + count] = k
            col_col[c:c + count] = np.arange(lo, lo + count)
            c += count
        stage.upload()
        with torch.cuda.device(self.device):
            for lo in range(0, ncols, MAX_COLS_PER_LAUNCH):
                n = min(MAX_COLS_PER_LAUNCH, ncols - lo)
                check(self.lib.w2l_mel_stream_cols(self.ctx, _lib.current_stream(), ptr(stage.dev), len(items),
                                                   stage.address(cols) + lo * MEL_COL.itemsize, n), "mel_stream_cols")


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
        if st.rs is not None:                 # the 16 kHz samples [buf_first, n16) lie in the stream's device buffer
            x, first = Resident(st.rs.buf, 0, st.rs.n16 - st.rs.buf_first), st.rs.buf_first
        else:
            x, first = st.samples(), st.held_first
        total = st.mel_samples() if st.mel_closed() else -1
        check_coverage(first, x.size, total, lo, count, st.key)
        items.append((x, first, total, st.window, st.cap, st.col0, lo, count))
        done.append((st, count))
    if items:
        mel.compute(items)
        for st, count in done:
            st.commit(count)
    return bool(items)


class DeviceResampler:
    """the device side of the incremental sample-rate conversion: 16 kHz buffers, the filter tables of every source rate
    (resident, `audio.resample_tables`), and one staged copy + one w2l_resample_stream launch per call"""

    def __init__(self, device):
        import torch
        from . import _lib
        self.torch, self.device, self.lib = torch, device, _lib.load()

    def new_buffer(self, cap16):
        return self.torch.zeros(cap16, dtype=self.torch.float32, device=self.device)

    @staticmethod
    def buffer_bytes(buf):
        return buf.numel() * buf.element_size()

    def compute(self, items):
        """items: (source samples float32 array, absolute index of [0], total or -1, n_res or -1, buffer, absolute 16 kHz index
        of buffer[0], its samples, carry or None, source rate, first output, count, time registers of the outputs).
        carry: (previous buffer, absolute index of its [0], first sample to copy, count) - the copy runs in the same launch"""
        from . import _lib, audio
        from ._lib import check, ptr
        torch, B = self.torch, RESAMPLE_BLOCK
        nblocks = sum((it[10] + B - 1) // B + ((it[7][3] + B - 1) // B if it[7] else 0) for it in items)
        stage = Staging(self.device)
        streams, blocks = stage.table(RESAMPLE_STREAM, len(items)), stage.table(RESAMPLE_BLOCKS, nblocks)
        src = [stage.place(it[0]) for it in items]
        stage.allocate()
        st, bt = stage.view(streams), stage.view(blocks)
        b = 0
        for k, (x, first, total, n_res, buf, buf_first, cap16, carry, rate, t0, count, tr) in enumerate(items):
            _, inc, scale, index_step, _ = resample_params(rate)
            win, delta = audio.resample_tables(self.device, rate, RATE16)
            old, old_first, c0, cn = carry if carry else (None, 0, 0, 0)
            st[k] = (stage.address(src[k]), first, total, n_res, buf.data_ptr(), buf_first, win.data_ptr(), delta.data_ptr(),
                     old.data_ptr() if cn else 0, old_first, scale, inc, x.size, cap16, index_step, win.numel(),
                     old.numel() if cn else 0, (0, 0, 0))
            mine = resample_blocks(k, t0, tr, c0, cn)
            bt[b:b + len(mine)] = mine
            b += len(mine)
        assert b == nblocks
        stage.upload()
        with torch.cuda.device(self.device):
            for lo in range(0, nblocks, MAX_BLOCKS_PER_LAUNCH):
                n = min(MAX_BLOCKS_PER_LAUNCH, nblocks - lo)
                check(self.lib.w2l_resample_stream(_lib.current_stream(), stage.host_address(streams), ptr(stage.dev), len(items),
                                                   stage.address(blocks) + lo * RESAMPLE_BLOCKS.itemsize, n, RESAMPLE_TABLE),
                      "resample_stream")


def resample_blocks(stream, t0, tr, carry_first=0, carry_count=0):
    """the block entries (RESAMPLE_BLOCKS) of one stream in a launch: copy blocks for the `carry_count` samples from
    `carry_first` on that a fresh buffer takes over, then compute blocks for the outputs t0 .. t0 + len(tr) - 1, each of up to 128
    consecutive outputs with the time register of its FIRST one; the kernel's thread j adds the increment j times to it"""
    B, count = RESAMPLE_BLOCK, len(tr)
    out = np.zeros((carry_count + B - 1) // B + (count + B - 1) // B, RESAMPLE_BLOCKS)
    b = 0
    for lo in range(0, carry_count, B):
        out[b] = (stream, min(B, carry_count - lo), carry_first + lo, 0.0, 1, 0)
        b += 1
    for lo in range(0, count, B):
        out[b] = (stream, min(B, count - lo), t0 + lo, tr[lo], 0, 0)
        b += 1
    return out


def check_resample_coverage(x_first, x_size, total, K, tr, key=None):
    """the held source samples [x_first, x_first + x_size) cover what the outputs with the time registers `tr` read; the kernel
    does not clamp (it would skip the output) - so this is checked before every launch.  The registers grow: the first output's
    left wing and the last one's right wing bound the rest."""
    a, b = resample_sample_range(tr[0], K, total)[0], resample_sample_range(tr[-1], K, total)[1]
    if a < x_first or b >= x_first + x_size:
        raise RuntimeError("stream %r: %d outputs read source samples [%d, %d], held are [%d, %d)"
                           % (key, len(tr), a, b, x_first, x_first + x_size))


def advance_samples(resampler, states):
    """one staged copy + one launch on `resampler` (a DeviceResampler): the final 16 kHz samples every stream of `states` with
    a source rate of its own has buffer room for, continuing a full buffer in a fresh one first (its tail is carried over in
    the same launch); False when no stream had any"""
    items, done = [], []
    for st in states:
        rs = st.rs
        p = rs.plan() if rs is not None else None
        if p is None:
            continue
        roll, t0, count, tr = p
        carry = None
        if roll is not None or rs.buf is None:
            fresh = resampler.new_buffer(rs.cap16)
            if roll is not None and rs.n16 > roll:
                carry = (rs.buf, rs.buf_first, roll, rs.n16 - roll)
            rs.buf, rs.buf_first = fresh, roll or 0
        x = rs.samples()
        total, n_res = (rs.n_src, rs.n_res) if rs.closed else (-1, -1)
        reading = count if n_res < 0 else max(0, min(count, n_res - t0))      # behind n_res: the padded zero, which reads nothing
        if reading:
            check_resample_coverage(rs.held_first, x.size, total, rs.K, tr[:reading], st.key)
        if x.size < 1:
            raise RuntimeError("stream %r: no source samples held for outputs [%d, %d)" % (st.key, t0, t0 + count))
        items.append((x, rs.held_first, total, n_res, rs.buf, rs.buf_first, rs.cap16, carry, rs.rate, t0, count, tr))
        done.append((rs, count, tr))
    if items:
        resampler.compute(items)
        for rs, count, tr in done:
            rs.commit(count, tr)
    return bool(items)


class LipsyncStreams:
    """many live audio streams through one generator in shared batches (module docstring).  `sink(key, frame_u8)` receives every
    stream's frames in row order, then `sink(key, None)`; without a sink the frames are collected in `self.frames[key]` (which
    `drain` returns).  `on_batch(rows)` receives each launched batch's [(key, row index)] including the padding rows."""

    def __init__(self, model, batch_size=128, depth=None, precision="f32", fps=25., sink=None, on_batch=None, mel_window=1024,
                 detector=None, pads=(0, 10, 0, 0), smooth_T=5, face_det_batch_size=16, resample_buffer=1 << 16, blend=None,
                 no_face_hold=None, face_track=None, color_match=None):
        from .face_detection.many import check_hold
        from .face_detection.track import check_track
        from .inference import check_blend, check_color_match
        from .models.wav2lip import check_precision
        self.hold = check_hold(no_face_hold)             # None, or G: frames without a face pass through (module docstring)
        self.track = check_track(face_track)             # None, or a FaceTrack: live streams follow one face
        self.precision = check_precision(precision)
        self.blend = check_blend(blend)                  # None, or (feather, top): every frame's face is blended in
        self.color_match = check_color_match(color_match)   # None, "mean" or "full": every prediction is matched to its crop
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        if mel_window < MIN_WINDOW:
            raise ValueError("mel_window must be at least %d columns" % MIN_WINDOW)
        if resample_buffer < MIN_BUFFER16:
            raise ValueError("resample_buffer must be at least %d samples" % MIN_BUFFER16)
        self.resample_buffer = int(resample_buffer)      # 16 kHz samples per stream opened at another rate
        self._resampler = None                           # DeviceResampler, once such a stream has something to convert
        self.resample_launches = 0                       # w2l_resample_stream staging copies + launches so far
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
        self._ready_boxed = 0                            # how many of them have a box: those are the rows that fill batches
        # (ticket, [(stream, row, None), and (stream, row, frame index) per pass-through row behind it]), oldest first
        self._pending = collections.deque()
        self._runner = self._mel = None
        self.launches = 0                                # w2l_mel_stream_cols staging copies + launches so far
        # ---- live streams only (`open_live`)
        from .face_detection.live import CARRY_ROWS
        self.detector, self.pads, self.smooth_T = detector, tuple(int(p) for p in pads), int(smooth_T)
        self.face_det_batch_size = int(face_det_batch_size)
        if len(self.pads) != 4:
            raise ValueError("pads must be (top, bottom, left, right)")
        if not 0 <= self.smooth_T <= CARRY_ROWS:
            raise ValueError("smooth_T must be in 0..%d" % CARRY_ROWS)
        if self.face_det_batch_size < 1:
            raise ValueError("face_det_batch_size must be at least 1")
        self.errors = {}                                 # key -> message of a live stream that ended on a frame (many.NO_FACE, ...)
        self.box_launches = 0                            # w2l_face_boxes_stream launches so far: at most one per step
        self._boxes = None                               # DeviceBoxes
        self._detecting = None                           # (ticket, [stream per item]) of the detection the last step launched
        self._slots, self._free_slots = {}, []           # carry slot per live stream whose video is under way

    # ---- the stream's life
    def open(self, key, frames, boxes, static=False, fps=None, *, sample_rate=RATE16):
        """sample_rate: the rate of the samples `feed` will bring; other than 16000 they are converted on the device"""
        if key in self._streams:
            raise ValueError("stream %r is already open" % (key,))
        resample_params(sample_rate)
        frames = list(frames)
        if not frames:
            raise ValueError("stream %r: no frames" % (key,))
        checked = []
        for f, b in zip(frames[:1] if static else frames, boxes):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError("stream %r: frames must be uint8 [H,W,3] arrays" % (key,))
            try:
                if b is None and self.hold is None:
                    raise ValueError("a frame without a box needs LipsyncStreams(no_face_hold=...)")
                checked.append(None if b is None else validate_boxes([b], f.shape[0], f.shape[1])[0])
            except ValueError as e:
                raise ValueError("stream %r: %s" % (key, e)) from None
        if len(checked) != (1 if static else len(frames)):
            raise ValueError("stream %r: one box per frame" % (key,))
        self._streams[key] = StreamState(key, frames, checked, static, self.fps if fps is None else fps, self.mel_window,
                                         sample_rate=int(sample_rate), cap16=self.resample_buffer)

    def open_live(self, key, fps=None, cycle=True, *, sample_rate=RATE16):
        """a stream whose video arrives with its audio: no frames and no boxes; `feed_frames` brings frames, the detector of
        the constructor finds the faces as they come.  cycle=False: the rows end with the video instead of cycling over it."""
        if self.detector is None:
            raise ValueError("stream %r: open_live needs LipsyncStreams(detector=...)" % (key,))
        if key in self._streams:
            raise ValueError("stream %r is already open" % (key,))
        resample_params(sample_rate)
        self._streams[key] = LiveState(key, self.fps if fps is None else fps, self.mel_window, cycle, sample_rate=int(sample_rate),
                                       cap16=self.resample_buffer)

    def _get_live(self, key):
        st = self._get(key)
        if not st.live:
            raise ValueError("stream %r was opened with its frames" % (key,))
        return st

    def feed_frames(self, key, frames):
        """uint8 [H,W,3] BGR host arrays, or one uint8 device tensor [n,H,W,3], of the stream's shape (the first frame fixes it)"""
        self._get_live(key).feed_frames(frames)

    def close_video(self, key):
        """end of video: the boxes that depend on it become final with the next tick, then the rows cycle over the frames"""
        st = self._get_live(key)
        if st.video_closed:
            raise ValueError("stream %r: its video is closed" % (key,))
        if st.n_frames == 0:
            raise ValueError("stream %r: no frames; its video stays open" % (key,))
        st.video_closed = True

    def _get(self, key):
        try:
            return self._streams[key]
        except KeyError:
            raise KeyError("no open stream %r" % (key,)) from None

    def feed(self, key, samples):
        """float32 1-D samples at 16 kHz; on a stream opened at another rate what a WAV of that rate decodes to: int16, int32,
        uint8, float32 or float64, 1-D or [n, channels] (`native_samples`)"""
        self._get(key).feed(samples)

    def close(self, key):
        st = self._get(key)
        if st.closed:
            raise ValueError("stream %r is closed" % (key,))
        # the length of the 16 kHz signal: librosa's ceil(N * ratio) for a stream at another rate
        n = st.n_fed if st.rs is None else int(np.ceil(st.rs.n_src * st.rs.ratio))
        if n < MIN_SAMPLES or final_columns(n, True) < mel_step_size:
            del self._streams[key]
            if n < MIN_SAMPLES:
                raise ValueError("stream %r: %d samples; the spectrogram's reflect padding needs more than %d" % (key, n, NFFT // 2))
            # lipsync() on such audio fails in w2l_mel_gather (T >= 16): the same exception type, at close
            raise RuntimeError("stream %r: %d samples give %d mel columns; the generator needs a window of %d"
                               % (key, n, final_columns(n, True), mel_step_size))
        st.end_audio()

    # ---- the tick
    def _backend(self):
        if self._runner is None:
            from .inference import _blend_kw, _color_kw
            self._runner = BatchRunner(self.model, self.batch_size, self.depth, self.precision, **_blend_kw(self.blend),
                                       **_color_kw(self.color_match))
            self._mel = DeviceMel(self._runner.device)
        if self._boxes is None and self.detector is not None:
            self._boxes = DeviceBoxes(self._runner.device, self.detector, self.pads, self.smooth_T, self.face_det_batch_size,
                                      **({} if self.hold is None else {"hold": self.hold}),
                                      **({} if self.track is None else {"track": self.track}))

    def _columns_round(self):
        converted = False
        if any(st.rs is not None for st in self._streams.values()):      # streams at 16 kHz: no launch, nothing built
            if self._resampler is None:
                self._resampler = DeviceResampler(self._runner.device)
            converted = advance_samples(self._resampler, self._streams.values())
            self.resample_launches += converted
        more = advance_columns(self._mel, self._streams.values())
        self.launches += more
        return more or converted

    def step(self, flush=False):
        """compute the newly final columns (one launch for all streams; more only while a stream's backlog exceeds its window),
        launch the full batches of ready rows - with `flush` the remainder too - and deliver the batches that have finished"""
        self._backend()
        self._collect_boxes()
        while True:
            more = self._columns_round()
            for st in self._streams.values():
                for row, fi, box, s in st.take_rows():
                    self._ready.append((st, row, fi, box, (st.window, st.cap, s - st.col0)))
                    self._ready_boxed += box is not None
            self._launch(False)
            if not more:
                break
        for st in [st for st in self._streams.values() if st.live and st.finished()]:
            self._end(st)                                # cycle=False: the video ended behind the last delivered row
        self._detect_round()
        if flush:
            self._launch(True)
        while self._pending and self._runner.ready(self._pending[0][0]):
            self._collect()

    # ---- live streams: the boxes of the previous tick in, the frames of this tick out
    def _end(self, st):
        """a live stream none of whose rows is under way leaves"""
        if self._streams.get(st.key) is st:
            del self._streams[st.key]
        st.frames = st.window = st.rs = None
        st.video, st.fresh = [], []
        self.sink(st.key, None)

    def _fail(self, st, message):
        """a frame ended the stream: the rows taken so far are delivered, then `sink(key, None)`; `errors[key]` says why"""
        self.errors[st.key] = st.error = message
        if not st.rows_done:
            st.rows_done, st.n_rows = True, st.next_row
        if self._streams.get(st.key) is st:
            del self._streams[st.key]
        st.fresh = []
        if st.finished():
            self._end(st)

    def _collect_boxes(self):
        """WAIT for the detection the previous step launched (an event, never a poll: what is ready when is a function of the
        call sequence) and append every stream's newly final boxes"""
        if self._detecting is None:
            return
        from .face_detection.many import NO_FACE
        (ticket, sts), self._detecting = self._detecting, None
        for st, res in zip(sts, self._boxes.collect(ticket)):
            boxes, (code, frame) = res[:2]
            if self._streams.get(st.key) is not st:      # it ended meanwhile
                continue
            if code == 1:
                self._fail(st, NO_FACE)
                continue
            if code == 2:
                self._fail(st, "frame %d: the device left the frame's box to the host - a non-finite or huge coordinate, where the "
                               "reference's int() raises too, or more candidates than its NMS holds" % frame)
                continue
            if code:
                self._fail(st, "internal error: w2l_face_boxes_stream did not follow this stream's segment (status %d): the device "
                               "copy of the segment table failed the kernel's bounds" % code)
                continue
            try:
                if len(res) > 2:                         # with a hold: a gap frame has no box
                    st.boxes += [validate_boxes([b], *st.shape)[0] if v else None for b, v in zip(boxes, res[2])]
                else:
                    st.boxes += validate_boxes(boxes, *st.shape) if len(boxes) else []
            except ValueError as e:
                self._fail(st, "frame %d..%d: %s" % (len(st.boxes), len(st.boxes) + len(boxes) - 1, e))
                continue
            if st.close_sent and len(st.boxes) == st.n_frames:
                st.video_done = True

    def _detect_round(self):
        """the frames fed since the last tick, and the videos closed since: one staged copy, the detector batches and ONE
        w2l_face_boxes_stream launch for all of them (DeviceBoxes.launch)"""
        for st in [st for st in self._slots if self._streams.get(st.key) is not st or st.close_sent]:
            self._free_slots.append(self._slots.pop(st))
        items, sts = [], []
        for st in self._streams.values():
            if not st.live or st.close_sent or not (st.n_fresh() or st.video_closed):
                continue
            if st not in self._slots:
                self._slots[st] = self._free_slots.pop() if self._free_slots else len(self._slots)
            items.append((st.fresh, st.shape[0], st.shape[1], self._slots[st], st.seen, st.video_closed))
            sts.append(st)
        if not items:
            return
        self._boxes.reserve(1 + max(it[3] for it in items))
        ticket = self._boxes.launch(items)
        self.box_launches += 1
        for st, chunks in zip(sts, ticket["chunks"]):
            for n, frames in chunks:
                st.video.append(FrameChunk(st.key, st.seen, frames))
                st.seen += n
            assert st.seen == st.n_frames
            st.fresh, st.close_sent = [], st.video_closed
        self._detecting = (ticket, sts)

    def _launch(self, flush):
        bs = self.batch_size
        while True:
            # pass-through rows at the front: in row order behind the newest batch in flight, else at once
            while self._ready and self._ready[0][3] is None:
                st, row, fi, _, _ = self._ready.popleft()
                if self._pending:
                    self._pending[-1][1].append((st, row, fi))
                else:
                    self._deliver(st, self._source_frame(st, fi))
            if not (self._ready_boxed >= bs or (flush and self._ready_boxed)):
                break
            rows, owners = [], []                        # up to bs rows with a box, and the pass-through rows among and behind them
            while self._ready and (len(rows) < bs or self._ready[0][3] is None):
                st, row, fi, box, mel = self._ready.popleft()
                owners.append((st, row, fi if box is None else None))
                if box is not None:
                    rows.append((st, row, fi, box, mel))
            n = len(rows)
            self._ready_boxed -= n
            size = bs if n == bs else bucket(n, bs)
            ticket = self._runner.submit([st.locate(fi) + (box, mel) for st, _, fi, box, mel in rows], pad_to=size)
            if self.on_batch is not None:
                self.on_batch([(st.key, row) for st, row, _, _, _ in rows] + [(rows[-1][0].key, rows[-1][1])] * (size - n))
            self._pending.append((ticket, owners))
            if len(self._pending) >= self.depth:
                self._collect()

    @staticmethod
    def _source_frame(st, fi):
        """the bytes of a stream's frame fi on the host: what a pass-through row delivers"""
        where, j = st.locate(fi)
        f = where.frames[j]
        return f.cpu().numpy() if hasattr(f, "data_ptr") else np.array(f)

    def _deliver(self, st, frame):
        self.sink(st.key, frame)
        st.delivered += 1
        st.release_delivered()
        if st.finished():
            if self._streams.get(st.key) is st:
                del self._streams[st.key]
            st.frames = st.window = st.rs = None
            self.sink(st.key, None)

    def _collect(self):
        item, owners = self._pending.popleft()
        generated = iter(self._runner.result(item))
        for st, _, fi in owners:
            self._deliver(st, next(generated) if fi is None else self._source_frame(st, fi))

    def drain(self):
        """close nothing; run and deliver everything that is ready or in flight"""
        self.step(flush=True)
        while self._detecting is not None:               # live streams: the boxes in flight may make rows ready
            self.step(flush=True)
        while self._pending:
            self._collect()
        return self.frames

    def device_bytes(self, key=None):
        """device memory held per stream between ticks: its spectrogram window (the staging of a tick is transient), of a
        stream at another rate than 16 kHz its buffer of converted samples, and of a live stream the frames resident on the device"""
        sts = list(self._streams.values() if key is None else [self._get(key)])
        return (sum(DeviceMel.window_bytes(st.window) for st in sts if st.window is not None)
                + sum(DeviceResampler.buffer_bytes(st.rs.buf) for st in sts if st.rs is not None and st.rs.buf is not None)
                + sum(ch.nbytes for st in sts if st.live for ch in st.video))


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
    p.add_argument('--live_video', default=False, action='store_true',
                   help='Feed the frames of every video as they become due with the audio and detect faces as they arrive')
    p.add_argument('--native_rate', default=False, action='store_true',
                   help="Feed every WAV at the file's own rate and format; it is converted to 16 kHz on the device as it streams")
    from .inference import add_blend_flags, add_color_match_flag, add_det_scale_flag, add_hold_flag, add_track_flags
    add_det_scale_flag(p)
    add_blend_flags(p)
    add_color_match_flag(p)
    add_hold_flag(p)
    add_track_flags(p)
    return p


def main(argv=None, state_dict=None):
    """feed every `--audio` in `--chunk_ms` slices round-robin to its `--face`, step after each round, write <outdir>/<k>.avi as
    each stream ends; returns the written paths in stream order.  With `--live_video` a video (not an image, no `--box`) is fed
    frame by frame as its audio goes by - floor(fps * samples fed / 16000) frames so far - and `face_detect` is never called.
    With `--native_rate` a WAV is not converted up front: its samples are fed as the file holds them, in `--chunk_ms` slices of
    its own rate, to a stream opened at that rate.  `state_dict` (S3FD weights) replaces face_detection/s3fd.pth."""
    import copy

    import torch
    from scipy.io import wavfile

    from . import audio, inference
    a = build_parser().parse_args(argv)
    blend = inference.blend_from_args(a)
    color_kw = inference._color_kw(inference.color_match_from_args(a))
    detect_kw = inference.detect_kw_from_args(a)         # `--no_face_hold G`, `--face_track PICK`
    if len(a.face) != len(a.audio):
        raise ValueError("%d --face for %d --audio: pass them in pairs" % (len(a.face), len(a.audio)))
    dev = torch.device("cuda", torch.cuda.current_device())
    detector = None
    if a.live_video or state_dict is not None:
        detector = inference.detector_from_args(a, dev, state_dict)
    jobs = []
    for k, (face, wav_path) in enumerate(zip(a.face, a.audio)):
        one = copy.copy(a)
        one.face = face
        if os.path.isfile(face) and inference.is_image_path(face):
            one.static = True
        frames, fps = inference.read_frames(one)
        if not wav_path.endswith('.wav'):
            raise ValueError("--audio %s: pass a .wav" % wav_path)
        live = a.live_video and a.box[0] == -1 and not one.static
        if live:
            boxes = None
        elif a.box[0] == -1:
            det = inference.face_detect(frames if not one.static else [frames[0]], detector=detector, pads=a.pads, nosmooth=a.nosmooth,
                                        batch_size=a.face_det_batch_size, precision=inference.CLI_PRECISION[a.face_det_precision],
                                        det_scale=a.face_det_scale, **detect_kw)
            boxes = [c for _, c in det]
        else:
            boxes = [tuple(a.box)] * len(frames)
        # --native_rate: the samples as the file holds them (int16 / int32 / uint8 / float, 1-D or [n, channels]) at its rate
        rate, wav = wavfile.read(wav_path) if a.native_rate else (RATE16, None)
        if rate == RATE16:                    # a 16 kHz stream takes float32 mono, as it always has
            wav = audio.load_wav(wav_path, RATE16)
        jobs.append(dict(key=k, frames=frames, fps=fps, boxes=boxes, static=one.static, wav=wav, rate=int(rate),
                         chunk=max(1, int(round(rate * a.chunk_ms / 1000.))),
                         audio=wav_path, out=os.path.join(a.outdir, "%d.avi" % k), pos=0, live=live, fed=0))
    os.makedirs(a.outdir, exist_ok=True)
    model = inference.load_model(a.checkpoint_path, dev)
    got = {j["key"]: [] for j in jobs}

    def sink(key, frame):
        if frame is not None:
            got[key].append(frame)
            return
        j = jobs[key]
        if key not in streams.errors:
            inference.write_result(j["out"], got.pop(key), j["fps"], j["audio"])

    streams = LipsyncStreams(model, batch_size=a.wav2lip_batch_size, precision=inference.CLI_PRECISION[a.precision], sink=sink,
                             detector=detector, pads=a.pads, smooth_T=0 if a.nosmooth else 5, face_det_batch_size=a.face_det_batch_size,
                             **inference._blend_kw(blend), **color_kw, **detect_kw)
    for j in jobs:
        if j["live"]:
            streams.open_live(j["key"], fps=j["fps"], sample_rate=j["rate"])
        else:
            streams.open(j["key"], j["frames"], j["boxes"], static=j["static"], fps=j["fps"], sample_rate=j["rate"])
    live = list(jobs)
    while live:
        for j in live:
            streams.feed(j["key"], j["wav"][j["pos"]:j["pos"] + j["chunk"]])
            j["pos"] += j["chunk"]
            if j["live"] and j["fed"] is not None:
                # the frames that have become due; the audio's end brings the rest of the video
                due = len(j["frames"]) if j["pos"] >= len(j["wav"]) else min(len(j["frames"]), int(j["fps"] * j["pos"] / float(j["rate"])))
                if due > j["fed"]:
                    streams.feed_frames(j["key"], j["frames"][j["fed"]:due])
                    j["fed"] = due
                if due == len(j["frames"]):
                    streams.close_video(j["key"])
                    j["fed"] = None
            if j["pos"] >= len(j["wav"]):
                streams.close(j["key"])
        streams.step()
        live = [j for j in live if j["pos"] < len(j["wav"]) and j["key"] not in streams.errors]      # a frame without a face ends it
    streams.drain()
    for key, message in streams.errors.items():
        raise ValueError("--face %s: %s" % (a.face[key], message))
    return [j["out"] for j in jobs]


if __name__ == '__main__':
    main()
