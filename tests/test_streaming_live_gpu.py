"""Live streams on the device: w2l_face_boxes_stream (csrc/detect.hip) against its host statement
`face_detection.live.stream_boxes_host` by equality - nine streams per launch between fence rows, three ways of cutting them
into ticks, the status rules and every refusal - and `LipsyncStreams.open_live` end to end on the seeded filelist clips: every
delivered frame against `face_detect` + the whole audio's spectrogram + `rows_inference` run through the generator, a clip without
a face, bounded memory with cycle=False, and the command line with `--live_video`."""
import os

import numpy as np
import pytest
import torch

from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

FH, FW = 40, 50
FENCE = 1000000
SENTINEL = -7
LENGTHS = [1, 2, 3, 4, 5, 6, 11, 70, 130]     # 130: carried rows ahead of two boundaries of the kernel's chunks of 64 frames
SLOTS = [1, 3, 4, 6, 7, 9, 10, 11, 2]         # of 12: slots 0, 5, 8 belong to nobody and must keep their sentinels
N_SLOTS = 12


# ---------------------------------------------------------------- w2l_face_boxes_stream
def _cuts(kind, n, rng):
    """frame counts per tick; the close comes with the last tick"""
    if kind == "whole":
        return [n]
    if kind == "each":
        return [1] * n
    cut, pos = [0] if rng.integers(2) else [], 0
    while pos < n:
        c = min(int(rng.choice([0, 1, 1, 2, 3, 7, 40])), n - pos)
        cut.append(c)
        pos += c
    return cut + ([0] if rng.integers(2) else [])          # a close on an empty tick


class _Table:
    """one launch: the segments' rows side by side in the arenas with a fence row of huge coordinates before, between and after
    them, output rows with a sentinel row between the segments, sentinel status rows behind the real ones"""

    def __init__(self, cuda, parts, T, carry):
        """parts: [(rects [n_new,4], slot, seen, closed)]"""
        from wav2lip_amd.face_detection import live
        from wav2lip_amd.face_detection.s3fd import RECT_FOUND
        R = sum(len(p[0]) for p in parts) + len(parts) + 1
        self.rects = np.full((R, 4), FENCE, np.int32)
        self.flags = np.full((R,), RECT_FOUND, np.int32)
        self.segs = np.zeros(len(parts), live.BOX_STREAM_SEGMENT)
        row, out = 1, 1
        for k, (rects, slot, seen, closed) in enumerate(parts):
            n = len(rects)
            self.rects[row:row + n] = np.asarray(rects, np.int32).reshape(n, 4)
            self.segs[k] = (row, n, FH, FW, slot, seen, int(closed), out)
            row += n + 1
            out += live.new_final_count(seen, n, closed, T) + 1
        self.n_out, self.T, self.cuda, self.carry = out, T, cuda, carry
        self.boxes = torch.full((out, 4), SENTINEL, dtype=torch.int32, device=cuda)
        self.status = torch.full((len(parts) + 2, 2), SENTINEL, dtype=torch.int32, device=cuda)

    def launch(self, pads, n_seg=None, T=None, segs_dev=None, null=None, expect_ok=True):
        from wav2lip_amd import _lib
        from wav2lip_amd._lib import current_stream, ptr
        lib = _lib.load()
        self.segs_dev = torch.from_numpy(self.segs.view(np.uint8).copy()).to(self.cuda)
        self.rects_dev, self.flags_dev = torch.from_numpy(self.rects).to(self.cuda), torch.from_numpy(self.flags).to(self.cuda)
        args = [self.segs.ctypes.data, ptr(self.segs_dev) if segs_dev is None else segs_dev, ptr(self.rects_dev), ptr(self.flags_dev),
                ptr(self.carry), ptr(self.boxes), ptr(self.status)]
        if null is not None:
            args[null] = None
        rc = lib.w2l_face_boxes_stream(current_stream(), len(self.segs) if n_seg is None else n_seg, args[0], args[1], args[2], args[3],
                                       len(self.rects), args[4], N_SLOTS, *pads, self.T if T is None else T, args[5], self.n_out, args[6])
        torch.cuda.synchronize()
        if expect_ok:
            assert rc == 0, lib.w2l_last_error()
        else:
            assert rc != 0 and b"face_boxes_stream" in lib.w2l_last_error()
        return self.boxes.cpu().numpy(), self.status.cpu().numpy()

    def check_fences(self, boxes, status, written):
        """`written`: [(out0, count)] of the segments that wrote; every other output row and the spare status rows are sentinels"""
        inside = np.zeros(len(boxes), bool)
        for out0, count in written:
            inside[out0:out0 + count] = True
        assert (boxes[~inside] == SENTINEL).all() and (status[len(self.segs):] == SENTINEL).all()
        assert np.abs(boxes[inside]).max(initial=0) < 1000                       # no fence row was read


def _new_carry(cuda):
    return torch.full((N_SLOTS, 64, 4), SENTINEL, dtype=torch.int32, device=cuda)


def _check_carry(carry, states):
    """a stream's slot starts with its last min(seen, max(T, 1)) raw rects; the rest of the table is untouched"""
    got = carry.cpu().numpy()
    for slot, state in states.items():
        held = np.asarray(state[1], np.int32).reshape(-1, 4)
        assert np.array_equal(got[slot, :len(held)], held)
    assert (got[[s for s in range(N_SLOTS) if s not in SLOTS]] == SENTINEL).all()


def _stream_ticks(cuda, lengths, kind, T, pads):
    """streams of these lengths (stream k in slot SLOTS[k]) in one launch per tick; integer inputs and one correctly rounded fp64
    division on both sides: equality.  The streams' boxes over all ticks are `many.host_boxes` of the whole videos."""
    from wav2lip_amd.face_detection import live, many
    rng = np.random.default_rng(1000 * T + 10 * len(kind) + pads[0])
    videos = [rng.integers(0, 71, (n, 4)).tolist() for n in lengths]              # beyond the 40 x 50 frame: both clips act
    cuts = [_cuts(kind, n, rng) for n in lengths]
    carry = _new_carry(cuda)
    states, pos, got = {}, [0] * len(videos), [[] for _ in videos]
    for t in range(max(len(c) for c in cuts)):
        live_now = [k for k in range(len(videos)) if t < len(cuts[k])]
        parts = [(videos[k][pos[k]:pos[k] + cuts[k][t]], SLOTS[k], pos[k], t == len(cuts[k]) - 1) for k in live_now]
        table = _Table(cuda, parts, T, carry)
        boxes, status = table.launch(pads)
        assert not status[:len(parts)].any()
        written = []
        for (rects, slot, seen, closed), seg, k in zip(parts, table.segs, live_now):
            want, states[slot] = live.stream_boxes_host(states.get(slot), rects, closed, FH, FW, pads, T)
            out0 = int(seg["out0"])
            assert np.array_equal(boxes[out0:out0 + len(want)], want), (t, k, seen, len(rects), closed)
            written.append((out0, len(want)))
            got[k].append(want)
            pos[k] += len(rects)
        table.check_fences(boxes, status, written)
        _check_carry(carry, states)
    for k, video in enumerate(videos):
        assert np.array_equal(np.concatenate(got[k]), many.host_boxes(video, FH, FW, pads, T))


@pytest.mark.parametrize("kind", ["whole", "each", "random"])
@pytest.mark.parametrize("T,pads", [(0, (0, 10, 0, 0)), (1, (0, 10, 0, 0)), (5, (0, 10, 0, 0)), (5, (-2, -10, -4, -3)), (64, (3, 10, 5, 7))])
def test_face_boxes_stream_is_the_host_statement_tick_by_tick(cuda, kind, T, pads):
    _stream_ticks(cuda, LENGTHS, kind, T, pads)


@pytest.mark.parametrize("kind", ["whole", "random"])
@pytest.mark.parametrize("T", [5, 64])
def test_face_boxes_stream_is_the_host_statement_past_the_ring_of_three_chunks(cuda, kind, T):
    """one stream of 200 frames: a tick of more than 192 frames reuses the kernel's ring, and random cuts carry rows across it"""
    _stream_ticks(cuda, [200], kind, T, (0, 10, 0, 0))


def test_face_boxes_stream_reports_no_face_and_host_rows_and_leaves_that_stream_as_it_was(cuda):
    from wav2lip_amd.face_detection import live
    from wav2lip_amd.face_detection.s3fd import RECT_HOST, RECT_NONE
    rng = np.random.default_rng(5)
    T, pads = 5, (0, 10, 0, 0)
    carry = _new_carry(cuda)
    first = [rng.integers(0, 71, (n, 4)).tolist() for n in (6, 3, 9, 70, 2)]
    table = _Table(cuda, [(r, SLOTS[k], 0, False) for k, r in enumerate(first)], T, carry)
    boxes, status = table.launch(pads)
    states = {}
    for k, r in enumerate(first):
        _, states[SLOTS[k]] = live.stream_boxes_host(None, r, False, FH, FW, pads, T)
    _check_carry(carry, states)
    before = carry.cpu().numpy().copy()
    second = [rng.integers(0, 71, (n, 4)).tolist() for n in (4, 70, 9, 5, 3)]
    table = _Table(cuda, [(r, SLOTS[k], len(first[k]), k == 4) for k, r in enumerate(second)], T, carry)
    # a "none" at new row i: (1, seen + i), the first one; a row that is neither wins over an earlier "none": (2, seen + its row)
    for k, i, f in ((1, 66, RECT_NONE), (1, 68, RECT_NONE), (2, 2, RECT_NONE), (2, 7, RECT_HOST), (2, 8, 12345), (3, 0, RECT_HOST)):
        table.flags[int(table.segs[k]["row0"]) + i] = f
    boxes, status = table.launch(pads)
    assert status[:5].tolist() == [[0, 0], [1, 3 + 66], [2, 9 + 7], [2, 70 + 0], [0, 0]]
    written = []
    for k, r in enumerate(second):
        if status[k, 0]:
            continue                                                              # no box written: check_fences sees sentinels there
        want, states[SLOTS[k]] = live.stream_boxes_host(states[SLOTS[k]], r, k == 4, FH, FW, pads, T)
        out0 = int(table.segs[k]["out0"])
        assert np.array_equal(boxes[out0:out0 + len(want)], want) and len(want) > 0
        written.append((out0, len(want)))
    table.check_fences(boxes, status, written)
    after = carry.cpu().numpy()
    for k in (1, 2, 3):
        assert np.array_equal(after[SLOTS[k]], before[SLOTS[k]])                  # its carry is left as it was
    _check_carry(carry, states)


def test_face_boxes_stream_refuses_bad_arguments_without_launching(cuda):
    rng = np.random.default_rng(6)
    carry = _new_carry(cuda)

    def fresh(**edit):
        t = _Table(cuda, [(rng.integers(0, 71, (4, 4)).tolist(), 1, 0, False), (rng.integers(0, 71, (6, 4)).tolist(), 3, 0, True)], 5, carry)
        for name, value in edit.items():
            t.segs[name][1] = value
        return t

    pads = (0, 10, 0, 0)
    runs = [fresh().launch(pads, null=k, expect_ok=False) for k in range(7)]                      # a NULL pointer, each in turn
    runs += [fresh().launch(pads, n_seg=n, expect_ok=False) for n in (0, -1)]
    runs += [fresh().launch(pads, T=T, expect_ok=False) for T in (-1, 65)]
    t = fresh()
    spare = torch.zeros(128, dtype=torch.uint8, device=cuda)                                      # a valid address that is not 16-byte aligned
    runs.append(t.launch(pads, segs_dev=spare.data_ptr() + 8, expect_ok=False))
    for edit in (dict(n_new=-1), dict(seen=-1), dict(slot=-1), dict(slot=N_SLOTS), dict(slot=1), dict(row0=100), dict(out0=100)):
        runs.append(fresh(**edit).launch(pads, expect_ok=False))
    for boxes, status in runs:
        assert (boxes == SENTINEL).all() and (status == SENTINEL).all()
    assert (carry.cpu().numpy() == SENTINEL).all()                                               # nothing ran
    boxes, status = fresh().launch(pads, T=64)
    assert status[:2].tolist() == [[0, 0], [0, 0]]


# ---------------------------------------------------------------- end to end
PADS = (0, 10, 0, 0)
DET_BATCH = 8


def _gen_state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


def _model(cuda):
    from wav2lip_amd import models
    m = models.Wav2Lip()
    m.load_state_dict(_gen_state_dict())
    return m.to(cuda).eval()


def _detector(cuda, **kw):
    from wav2lip_amd import face_detection
    return face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(cuda),
                                        state_dict=synth.s3fd_state_dict(), **kw)


def _wav(pcm):
    return (pcm[:, 0].astype(np.float32) / 32768.0).astype(np.float32)


def _feed_live(ls, clips, slices, cycle=True):
    """per tick every clip gets `slices[name]` frames and as many 40 ms of its audio; the video closes with its last frame"""
    pos = dict.fromkeys(clips, 0)
    for name in clips:
        ls.open_live(name, cycle=cycle)
    while any(name in ls._streams for name in clips):
        for name, (frames, wav) in clips.items():
            if name not in ls._streams:
                continue
            k, p = slices[name], pos[name]
            if p * 640 < len(wav):
                ls.feed(name, wav[p * 640:(p + k) * 640])
            if p < len(frames):
                ls.feed_frames(name, list(frames[p:p + k]))
                if p + k >= len(frames):
                    ls.close_video(name)
            pos[name] = p + k
            if pos[name] * 640 >= len(wav) and not ls._streams[name].closed:
                ls.close(name)
        ls.step()
        if all(name not in ls._streams or (pos[name] * 640 >= len(clips[name][1]) and pos[name] >= len(clips[name][0])) for name in clips):
            break                                                                 # everything is fed: the rest is `drain`'s
    ls.drain()


def _whole_batch_boxes(det, frames):
    """`face_detect` as a live stream defines it: the detector on whole batches of DET_BATCH frames, the last one padded with its
    last frame (a live tick pads with its last address), then `face_detect`'s finish on all rects"""
    from wav2lip_amd.face_detection import many
    rects = []
    for lo in range(0, len(frames), DET_BATCH):
        batch = list(frames[lo:lo + DET_BATCH])
        n = len(batch)
        rects += det.get_detections_for_batch(np.array(batch + [batch[-1]] * (DET_BATCH - n)))[:n]
    if any(r is None for r in rects):
        raise ValueError(many.NO_FACE)
    H, W = frames[0].shape[:2]
    return [tuple(int(v) for v in b) for b in many.host_boxes(rects, H, W, PADS, 5)]


def _reference_boxes(det, frames, setting):
    """the boxes a live stream of `frames` must have.  With the fp32 detector (whole or reduced frame): `face_detect` as it is,
    ragged last batch included.  With the bf16 detector the launches depend on the batch size (tests/test_streaming_live_cpu.py
    shows the split-K factors of a batch of 7 and of 8), so the contract is `face_detect` in whole batches; how many boxes the
    ragged `face_detect` gives differently is printed (on an MI355X: 0 of 39, 0 of 61, 4 of 52, and 1 of c4's first 7)."""
    from wav2lip_amd import inference
    ragged = [c for _, c in inference.face_detect(list(frames), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH)]
    if setting != "bf16":
        return ragged
    whole = _whole_batch_boxes(det, frames)
    print("bf16 detector, %d frames: %d boxes of the ragged face_detect differ from detection in whole batches of %d"
          % (len(frames), sum(tuple(a) != tuple(b) for a, b in zip(ragged, whole)), DET_BATCH))
    return whole


@pytest.mark.parametrize("setting", ["f32", "bf16", "scale2"])
def test_live_streams_deliver_face_detect_plus_lipsync_of_the_whole_clips(cuda, setting):
    """c0, c1 and c3 in 1-, 3- and 7-frame slices with their audio, c4 (a frame without a face) among them; none of the clips is
    a whole number of detector batches.  The reference per clip is made from the WHOLE inputs: `_reference_boxes` on all frames
    (the same detector), the spectrogram of all samples, `rows_inference`.  Those rows go through the generator in the batches
    the streams recorded (`multiclip.BatchRunner`, as tests/test_streaming_gpu.py replays them): byte for byte.  In fp32 each
    clip also runs alone through `multiclip.lipsync_many`, whose batches are composed differently; there the bar is the one of
    test_streamed_frames_against_lipsync_on_the_whole_audio, and the differing bytes are printed."""
    from wav2lip_amd import audio, inference, multiclip, streaming
    from wav2lip_amd.face_detection import many
    src = synth.filelist_clips()
    clips = {name: (src[name][0], _wav(src[name][1])) for name in ("c0", "c4", "c1", "c3")}
    slices = {"c0": 1, "c4": 3, "c1": 3, "c3": 7}
    assert all(len(f) % DET_BATCH for f, _ in clips.values())
    det = _detector(cuda, **{"f32": {}, "bf16": dict(precision="bf16"), "scale2": dict(det_scale=2)}[setting])
    model = _model(cuda)
    batches, out = [], {name: [] for name in clips}
    ls = streaming.LipsyncStreams(model, batch_size=16, on_batch=batches.append, detector=det, pads=PADS, face_det_batch_size=DET_BATCH,
                                  sink=lambda k, f: out[k].append(f) if f is not None else None)
    _feed_live(ls, clips, slices)
    assert ls.errors == {"c4": many.NO_FACE} and not ls._streams and ls.device_bytes() == 0
    # c4 in 3-frame slices: the tick of frames 3..5 makes boxes 0 and 1 final, the next tick brings the faceless frame 7
    assert len(out["c4"]) == 2
    jobs, rows = {}, {}
    for name, (frames, wav) in clips.items():
        mel = audio.melspectrogram_device(wav, cuda)
        if name == "c4":
            with pytest.raises(ValueError, match="Face not detected"):
                inference.face_detect(list(frames), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH)
            # the rows it did deliver: box i <= n - T looks forward only, so the first 3 boxes of frames [0, 7) are those rows'
            # boxes whatever follows
            boxes = _reference_boxes(det, frames[:7], setting)
            rows[name] = multiclip.rows_inference(mel.shape[1], 7, boxes, 25.)[:len(out[name])]
            jobs[name] = multiclip.ClipJob(name, list(frames), mel, rows[name])
            continue
        boxes = _reference_boxes(det, frames, setting)
        rows[name] = multiclip.rows_inference(mel.shape[1], len(frames), boxes, 25.)
        jobs[name] = multiclip.ClipJob(name, list(frames), mel, rows[name])
        assert len(out[name]) == len(rows[name]) > 0
    assert len({rows["c1"][i][1] for i in range(len(rows["c1"]))}) > 1           # the boxes do move from frame to frame
    runner = multiclip.BatchRunner(model, 16, 2, "f32")
    seen = dict.fromkeys(clips, 0)
    for rec in batches:
        real = list(dict.fromkeys(rec))
        item = runner.submit([(jobs[k], rows[k][i][0], rows[k][i][1], rows[k][i][2]) for k, i in real], pad_to=len(rec))
        for (k, i), f in zip(real, runner.result(item)):
            assert i == seen[k] and np.array_equal(out[k][i], f), (setting, k, i)
            seen[k] += 1
    assert seen == {k: len(rows[k]) for k in clips}
    if setting != "f32":
        return
    for name, job in jobs.items():
        if name == "c4":
            continue
        ref = multiclip.lipsync_many(model, [job], batch_size=16)[name]
        d = [np.abs(a.astype(np.int32) - b.astype(np.int32)) for a, b in zip(out[name], ref)]
        worst, differing = max(int(x.max()) for x in d), sum(int((x != 0).sum()) for x in d)
        print("clip %s: %d rows, against lipsync_many alone: max difference %d, %d of %d bytes differ"
              % (name, len(ref), worst, differing, sum(x.size for x in d)))
        assert len(ref) == len(out[name]) and worst <= 1


def test_cycle_false_holds_no_more_frames_at_the_end_of_a_long_stream_than_in_its_middle(cuda):
    from wav2lip_amd import streaming
    frames = synth.filelist_clips()["c1"][0]
    frames = np.concatenate([frames[:60]] * 3)                                    # 180 frames of 128 x 144
    wav = synth.noise_wav(640 * 190, seed=5)
    det, model = _detector(cuda), _model(cuda)
    n_out = [0]
    ls = streaming.LipsyncStreams(model, batch_size=16, detector=det, pads=PADS, face_det_batch_size=DET_BATCH, mel_window=64,
                                  sink=lambda k, f: n_out.__setitem__(0, n_out[0] + (f is not None)))
    ls.open_live("s", cycle=False)
    held = {}
    for t in range(60):
        ls.feed("s", wav[t * 1920:(t + 1) * 1920])
        ls.feed_frames("s", list(frames[3 * t:3 * t + 3]))
        ls.step(flush=True)
        while ls._pending:
            ls._collect()                                                         # after delivery
        held[t] = ls.device_bytes("s")
    frame_bytes = 128 * 144 * 3
    print("device bytes held after ticks 10, 30, 59: %d, %d, %d (%d-byte frames)" % (held[10], held[30], held[59], frame_bytes))
    assert held[59] <= held[30] <= 80 * 64 * 4 + 16 * frame_bytes
    ls.close_video("s")
    ls.feed("s", wav[60 * 1920:])
    ls.close("s")
    ls.drain()
    assert n_out[0] == 180 and not ls._streams and not ls.errors


def test_live_video_flag_writes_the_same_avi_bytes(cuda, tmp_path):
    from scipy.io import wavfile
    from wav2lip_amd import container, streaming
    src = synth.filelist_clips()
    argv = ["--checkpoint_path", str(tmp_path / "ckpt.pth"), "--wav2lip_batch_size", "16", "--face_det_batch_size", str(DET_BATCH)]
    for i, name in enumerate(("c0", "c1")):
        frames, pcm = src[name]
        container.write_avi(str(tmp_path / ("v%d.avi" % i)), frames, 25)
        wavfile.write(str(tmp_path / ("a%d.wav" % i)), 16000, pcm[:, 0])
        argv += ["--face", str(tmp_path / ("v%d.avi" % i)), "--audio", str(tmp_path / ("a%d.wav" % i))]
    torch.save({"state_dict": {"module." + k: v for k, v in _gen_state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp_path / "ckpt.pth"))
    sd = synth.s3fd_state_dict()
    plain = streaming.main(argv + ["--outdir", str(tmp_path / "plain")], state_dict=sd)
    with pytest.MonkeyPatch.context() as mp:
        from wav2lip_amd import inference

        def never(*a, **k):
            raise AssertionError("--live_video must not call face_detect")
        mp.setattr(inference, "face_detect", never)
        live = streaming.main(argv + ["--outdir", str(tmp_path / "live"), "--live_video"], state_dict=sd)
    assert [os.path.basename(p) for p in live] == [os.path.basename(p) for p in plain] == ["0.avi", "1.avi"]
    for a, b in zip(plain, live):
        assert len(container.read_avi(a)["frames"]) > 30
        assert open(a, "rb").read() == open(b, "rb").read()
