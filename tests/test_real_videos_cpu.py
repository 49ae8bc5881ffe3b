"""ReSyncED generation without a device (wav2lip_amd/real_videos_inference.py): the four host rules against the tables of the
executed reference (tests/golden/golden_real_videos_v1.npz, tests/golden/make_golden_real_videos.py), the command-line surface,
and the producer with the device steps stubbed at their seams and the generator at the `BatchRunner` seam: pairing and order in
`dubbed` mode, the numbering after a skipped clip, the frame / audio mismatch per mode, `tts` duplicates as rows, lazy
consumption, and a device-tensor job that stages no frame bytes."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from wav2lip_amd import synthetic as synth

G = np.load(os.path.join(ROOT, "tests", "golden", "golden_real_videos_v1.npz"))


def test_increase_frames_index_equals_the_executed_reference_over_the_grid():
    from wav2lip_amd import real_videos_inference as rv
    flat, at = G["increase_index"].tolist(), 0
    assert len(G["increase_grid"]) > 60
    for n, l in G["increase_grid"].tolist():
        got = rv.increase_frames_index(n, l)
        assert got == flat[at:at + l], (n, l)
        at += l
        assert len(got) == l and all(a <= b for a, b in zip(got, got[1:])) and (l == 0 or (0 <= got[0] and got[-1] < n)), (n, l)
    assert at == len(flat)
    assert rv.increase_frames_index(7, 3) == [0, 1, 2] and rv.increase_frames_index(5, 5) == list(range(5))
    with pytest.raises(ValueError):
        rv.increase_frames_index(0, 4)


def test_rescale_factor_equals_the_executed_reference_over_the_grid():
    from wav2lip_amd import real_videos_inference as rv
    got = [rv.rescale_factor(face, h, w, face_res, min_res) for face, h, w, face_res, min_res in G["factor_grid"].tolist()]
    assert got == G["factor_table"].tolist()
    assert len(set(got)) >= 5 and min(got) == 1 and max(got) == 14


def test_real_chunk_starts_equal_the_executed_loop_at_three_frame_rates():
    from wav2lip_amd import real_videos_inference as rv
    assert G["chunk_fps"].tolist() == [25., 30., 23.976]
    for k, fps in enumerate(G["chunk_fps"].tolist()):
        for n_mel in G["chunk_n_mel"].tolist():
            want = G["chunks_%d_%d" % (k, n_mel)].tolist()
            assert rv.real_chunk_starts(n_mel, fps) == want, (fps, n_mel)
            assert not want or want[-1] + 16 <= n_mel                              # full windows only, no tail window
    assert rv.real_chunk_starts(15, 25.) == [] and rv.real_chunk_starts(16, 25.) == [0]


def test_capped_size_equals_the_sizes_the_reference_resized_to():
    from wav2lip_amd import real_videos_inference as rv
    flags = json.loads(str(G["flags"]))
    max_res = int(flags[flags.index("--max_frame_res") + 1])
    fired = 0
    for (h, w), (hc, wc) in zip(G["size_read"].tolist(), G["size_capped"].tolist()):
        cap = rv.capped_size(h, w, max_res)
        if (h, w) == (hc, wc):
            assert cap is None
        else:
            assert cap == (wc, hc)
            fired += 1
    assert fired >= 2
    assert rv.capped_size(720, 1280, 720) is None and rv.capped_size(1080, 1920, 720) == (1280, 720)
    assert rv.capped_size(1280, 721, 720) == (int(721 / (721 / 720.)), int(1280 / (721 / 720.)))


def _surface(parser):
    rows = []
    for a in parser._actions:
        if a.dest == "help":
            continue
        rows.append([list(a.option_strings), a.dest, getattr(a.type, "__name__", None), a.default, a.nargs, bool(a.required),
                     type(a).__name__])
    return rows


def test_cli_surface_is_the_references_with_typed_resolutions_plus_the_two_precision_flags():
    from wav2lip_amd import real_videos_inference as rv
    ref = json.loads(str(G["cli"]))
    assert [r[1] for r in ref] == ["mode", "filelist", "results_dir", "data_root", "checkpoint_path", "pads", "face_det_batch_size",
                                   "wav2lip_batch_size", "face_res", "min_frame_res", "max_frame_res"]
    ours = _surface(rv.parser)
    typed = {"face_res", "min_frame_res", "max_frame_res"}
    for a, b in zip(ours, ref):
        if b[1] in typed:                               # the one deliberate difference: the reference declares no type
            assert b[2] is None and a[2] == "int" and a[:2] + a[3:] == b[:2] + b[3:]
        else:
            assert a == b
    assert len(ours) == len(ref)
    cli = _surface(rv.cli_parser)
    assert cli[:len(ref)] == ours and [r[1] for r in cli[len(ref):]] == ["precision", "face_det_precision"]
    a = rv.cli_parser.parse_args(["--mode", "tts", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c", "--face_res", "90"])
    assert (a.pads, a.face_det_batch_size, a.wav2lip_batch_size, a.face_res, a.min_frame_res, a.max_frame_res, a.filelist,
            a.precision, a.face_det_precision) == ([0, 10, 0, 0], 16, 128, 90, 480, 720, None, "fp32", "fp32")


# ---------------------------------------------------------------- the producer, device steps stubbed
class StubRunner:
    """BatchRunner without a device: a batch's "output" frames are its rows' input frames"""
    instances = []

    def __init__(self, model, batch_size, depth, precision):
        self.batches = []
        StubRunner.instances.append(self)

    def submit(self, rows):
        self.batches.append([(job.key, fi, box, start) for job, fi, box, start in rows])
        return [np.asarray(job.frames[fi]).copy() for job, fi, _, _ in rows]

    def result(self, item):
        return item


def _mel_columns(chunks, fps=25.):
    return int((chunks - 1) * 80. / fps) + 16


@pytest.fixture
def seams(monkeypatch):
    """clips: name -> (frames, fps, chunks of its audio); every device step replaced by a host stand-in that records its calls"""
    from wav2lip_amd import multiclip, real_videos_inference as rv
    StubRunner.instances = []
    monkeypatch.setattr(multiclip, "BatchRunner", StubRunner)
    calls = {"read": [], "upload": [], "resize": [], "boxes": [], "no_face": set()}
    clips = {}

    def read_inputs(video, audio_src, tmpdir):
        v, a = (os.path.basename(p)[:-len(".avi")] for p in (video, audio_src))
        calls["read"].append((v, a))
        frames, fps, _ = clips[v]
        chunks = clips[a][2]
        pcm = np.full((100, 1), hash(a) % 1000, np.int16)
        return frames, fps, types.SimpleNamespace(columns=_mel_columns(chunks, fps)), pcm, 16000

    def upload_frames(frames, device):
        calls["upload"].append(len(frames))
        return torch.from_numpy(np.ascontiguousarray(frames))

    def resize_frames_device(frames, wh):
        calls["resize"].append((tuple(frames.shape[1:3]), tuple(wh)))
        return torch.zeros((frames.shape[0], wh[1], wh[0], 3), dtype=torch.uint8)

    def first_rect(detector, frames):
        return None if int(frames[0, 0, 0, 0]) in calls["no_face"] else (2, 1, 8, 11)

    def clip_boxes(detector, frames, index, pads, batch_size):
        calls["boxes"].append(list(index))
        return np.asarray([(1, 9, 2, 8)] * len(index))

    monkeypatch.setattr(rv, "read_inputs", read_inputs)
    monkeypatch.setattr(rv, "upload_frames", upload_frames)
    monkeypatch.setattr(rv, "resize_frames_device", resize_frames_device)
    monkeypatch.setattr(rv, "first_rect", first_rect)
    monkeypatch.setattr(rv, "clip_boxes", clip_boxes)
    monkeypatch.setattr(rv, "device_mel", lambda wav, device: types.SimpleNamespace(shape=(80, wav.columns)))
    return rv, clips, calls


def _clip(tag, n_frames, chunks, shape=(12, 10), fps=25.):
    frames = np.zeros((n_frames,) + shape + (3,), np.uint8)
    frames[:, 0, 0, 0] = tag
    frames[:, 0, 0, 1] = np.arange(n_frames)
    return frames, fps, chunks


def _args(rv, tmp_path, mode, extra=()):
    return rv.cli_parser.parse_args(["--mode", mode, "--results_dir", str(tmp_path / "out"), "--data_root", str(tmp_path / "data"),
                                     "--checkpoint_path", "none", "--wav2lip_batch_size", "8", "--filelist", str(tmp_path / "l.txt")]
                                    + list(extra))


RANKS = types.SimpleNamespace(rank=0, world=1, device="cpu")


def _run(rv, args, lines, report=None):
    os.makedirs(args.results_dir, exist_ok=True)
    return rv.run(args, lines, RANKS, None, None, report)


def test_dubbed_mode_pairs_every_file_with_itself_in_sorted_order(seams, tmp_path):
    from wav2lip_amd import container
    rv, clips, calls = seams
    os.makedirs(str(tmp_path / "data"))
    for k, name in enumerate(("zeta", "alpha", "mid")):
        open(str(tmp_path / "data" / (name + ".avi")), "wb").close()
        clips[name] = _clip(10 + k, 6, 5)
    args = _args(rv, tmp_path, "dubbed")
    lines = rv.lines_of(args)
    assert lines == ["alpha.avi alpha.avi", "mid.avi mid.avi", "zeta.avi zeta.avi"]
    assert _run(rv, args, lines) == [0, 1, 2]
    assert calls["read"] == [("alpha", "alpha"), ("mid", "mid"), ("zeta", "zeta")]
    assert sorted(os.listdir(args.results_dir)) == ["0.avi", "1.avi", "2.avi"]
    got = container.read_avi(os.path.join(args.results_dir, "2.avi"))
    assert len(got["frames"]) == 5 and int(got["frames"][0, 0, 0, 0]) == 10 and got["fps"] == 25.0      # zeta's frames, truncated
    assert np.array_equal(got["audio"], np.full((100, 1), hash("zeta") % 1000, np.int16))


def test_a_skipped_clip_leaves_a_gap_in_the_numbering(seams, tmp_path):
    rv, clips, calls = seams
    clips.update(a=_clip(1, 5, 5), b=_clip(2, 5, 5), c=_clip(3, 9, 7, fps=30.))
    calls["no_face"].add(2)
    args = _args(rv, tmp_path, "random")
    assert _run(rv, args, ["a a\n", "b a\n", "c c\n"]) == [0, 2]
    assert sorted(os.listdir(args.results_dir)) == ["0.avi", "2.avi"]
    assert calls["read"] == [("a", "a"), ("b", "a"), ("c", "c")]                     # `video audio_src`: the video comes first
    assert calls["upload"] == [5, 5, 7]                                              # frames beyond the chunk count never go up


@pytest.mark.parametrize("mode", ["random", "dubbed"])
def test_fewer_frames_than_chunks_is_the_references_error_outside_tts_mode(seams, tmp_path, mode):
    rv, clips, calls = seams
    clips.update(a=_clip(1, 5, 5), short=_clip(2, 4, 9))
    args = _args(rv, tmp_path, mode)
    with pytest.raises(ValueError, match="#Frames, audio length mismatch"):
        _run(rv, args, ["a a\n", "short short\n", "a a\n"])
    assert calls["read"] == [("a", "a"), ("short", "short")]                         # not caught: the run ends there


def test_tts_mode_names_frames_twice_and_copies_none(seams, tmp_path):
    from wav2lip_amd import container
    rv, clips, calls = seams
    clips.update(short=_clip(2, 4, 10), a=_clip(1, 6, 5))
    args = _args(rv, tmp_path, "tts")
    report = {}
    assert _run(rv, args, ["short short\n", "a a\n"], report) == [0, 1]
    want = rv.increase_frames_index(4, 10)
    assert report[0]["index"] == want and len(set(want)) == 4 and report[1]["index"] == list(range(5))
    assert calls["upload"] == [4, 5] and calls["boxes"] == [want, list(range(5))]    # four frames went up for ten rows
    rows = [r for b in StubRunner.instances[-1].batches for r in b]
    assert [fi for k, fi, _, _ in rows if k == 0] == want                            # a duplicate is a second row on the same frame
    assert [len(b) for b in StubRunner.instances[-1].batches] == [8, 7]              # rows of both clips share a batch
    got = container.read_avi(os.path.join(args.results_dir, "0.avi"))["frames"]
    assert got[:, 0, 0, 1].tolist() == want


def test_both_resizes_are_asked_for_with_the_references_sizes(seams, tmp_path):
    rv, clips, calls = seams
    clips.update(big=_clip(1, 3, 3, shape=(180, 240)))
    args = _args(rv, tmp_path, "random", ["--max_frame_res", "144", "--min_frame_res", "60", "--face_res", "4"])
    report = {}
    _run(rv, args, ["big big\n"], report)
    # the stub's first rect is 10 pixels high: factor 2 brings it to 5, closer to 4; factor 3 would take the frame below 60
    assert calls["resize"] == [((180, 240), (192, 144)), ((144, 192), (96, 72))]
    assert report[0]["read"] == (180, 240) and report[0]["capped"] == (144, 192) and report[0]["rescaled"] == (72, 96)
    assert report[0]["factor"] == 2


def test_jobs_are_produced_lazily(seams, tmp_path):
    rv, clips, calls = seams
    for k in range(30):
        clips["c%d" % k] = _clip(k, 4, 4)
    args = _args(rv, tmp_path, "random")
    os.makedirs(args.results_dir, exist_ok=True)
    tracks = {}
    gen = rv.clip_jobs(args, ["c%d c%d\n" % (k, k) for k in range(30)], RANKS, None, tracks)
    first = next(gen)
    assert first.key == 0 and len(calls["read"]) == 1 and isinstance(first.frames, torch.Tensor)
    gen.close()
    calls["read"].clear()
    seen = []

    class Sink(rv.ResultSink):
        def __call__(self, idx, frame):
            if frame is None:
                seen.append((idx, len(calls["read"])))
            rv.ResultSink.__call__(self, idx, frame)

    from wav2lip_amd import multiclip
    tracks = {}
    sink = Sink(args.results_dir, tracks)
    multiclip.lipsync_many(None, rv.clip_jobs(args, ["c%d c%d\n" % (k, k) for k in range(30)], RANKS, None, tracks), batch_size=8,
                           depth=2, sink=sink)
    assert [i for i, _ in seen] == list(range(30))
    # batches of 8 rows = 2 clips, 2 in flight: when clip i closes, the producer has read at most the clips of 3 batches more
    assert all(read - (i + 1) <= 3 * 2 + 1 for i, read in seen), seen


def test_a_device_tensor_job_stages_no_frame_bytes():
    from wav2lip_amd import multiclip, staging
    mel = types.SimpleNamespace(shape=(80, 100))
    host = np.zeros((4, 12, 10, 3), np.uint8)
    resident = torch.zeros((4, 12, 10, 3), dtype=torch.uint8)
    rows = [(0, (1, 9, 2, 8), 0), (0, (1, 9, 2, 8), 3), (3, (1, 9, 2, 8), 6)]          # frame 0 twice
    tables = staging.align(3 * multiclip.FRAME_ROW.itemsize) + staging.align(3 * multiclip.MEL_ROW.itemsize)
    for frames, staged in ((host, 2), (resident, 0)):
        job = multiclip.ClipJob("k", frames, mel, rows)
        checked = multiclip._checked_rows(job)
        assert checked == rows
        off, mel_off, src_off, staged_frames, out_off, out_bytes = multiclip.staging_layout([(job,) + r for r in checked], 3)
        assert len(staged_frames) == len(src_off) == staged
        assert off == tables + staged * 368                                          # resident: only the two tables travel
        assert out_off == [0, 368, 736] and out_bytes == 3 * 368                     # outputs come back either way
    for bad_rows, what in (([(4, (1, 9, 2, 8), 0)], "frame index"), ([(0, (1, 13, 2, 8), 0)], "outside"), ([(0, (1, 9, 2, 8), 90)], "mel window")):
        with pytest.raises(ValueError, match=what):
            multiclip._checked_rows(multiclip.ClipJob("k", resident, mel, bad_rows))
    with pytest.raises(ValueError, match="contiguous uint8"):
        multiclip._checked_rows(multiclip.ClipJob("k", resident[:, :, ::2], mel, rows))
    with pytest.raises(ValueError, match="contiguous uint8"):
        multiclip._checked_rows(multiclip.ClipJob("k", resident.float(), mel, rows))
