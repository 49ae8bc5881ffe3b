"""Host side of the filelist generation path (wav2lip_amd/multiclip.py, wav2lip_amd/gen_videos_from_filelist.py): the two row
conventions against the executed reference (tests/golden/golden_filelist_v1.npz) and `mel_chunk_starts`, the packer with its
device side stubbed at the `BatchRunner` seam, the command-line surface and the dealing of lines to ranks."""
import json
import os
import types

import numpy as np
import pytest

from conftest import ROOT
from wav2lip_amd import synthetic as synth

G = np.load(os.path.join(ROOT, "tests", "golden", "golden_filelist_v1.npz"))


def _mel_columns(n_chunks):
    return 1 + synth.filelist_samples(n_chunks) // 200


def test_rows_filelist_gives_the_references_chunk_counts_and_frame_indices():
    from wav2lip_amd import multiclip
    clips = {name: (t, chunks) for name, _, t, chunks, _ in synth.FILELIST_CLIPS}
    for idx, (a, v) in enumerate(synth.FILELIST_LINES):
        n_frames, chunks = clips[v][0], clips[a][1]
        boxes = [(0, 8, 0, 8)] * n_frames
        if n_frames < chunks:
            assert int(G["written"][idx]) == 0
            with pytest.raises(ValueError, match="fewer|shorter"):
                multiclip.rows_filelist(_mel_columns(chunks), n_frames, boxes)
            continue
        rows = multiclip.rows_filelist(_mel_columns(chunks), n_frames, boxes)
        assert len(rows) == chunks
        if int(G["written"][idx]):
            assert len(rows) == int(G["n_frames"][idx])
        assert [r[0] for r in rows] == list(range(chunks))                     # chunk i on frame i: no cycling, no tail window
        assert [r[2] for r in rows] == [int(i * 3.2) for i in range(chunks)]
        assert rows[-1][2] + 16 <= _mel_columns(chunks)
    assert multiclip.rows_filelist(15, 4, [(0, 1, 0, 1)] * 4) == []             # no full window


def test_rows_inference_follows_mel_chunk_starts_and_cycles_frames():
    from wav2lip_amd import inference, multiclip
    for T, fps, nf in ((241, 25., 5), (170, 30., 200), (16, 25., 1)):
        boxes = [(k, k + 4, 0, 4) for k in range(nf)]
        rows = multiclip.rows_inference(T, nf, boxes, fps)
        starts = inference.mel_chunk_starts(T, fps)
        assert [r[2] for r in rows] == starts and rows[-1][2] == T - 16         # the tail window is re-anchored
        assert [r[0] for r in rows] == [i % nf for i in range(len(starts))]
        assert all(r[1] == boxes[r[0]] for r in rows)
        assert {r[0] for r in multiclip.rows_inference(T, nf, boxes, fps, static=True)} == {0}


class StubRunner:
    """BatchRunner without a device: a batch's "output" frames are its rows' input frames"""
    instances = []

    def __init__(self, model, batch_size, depth, precision):
        self.batches, self.live = [], []
        self.args = (batch_size, depth, precision)
        StubRunner.instances.append(self)

    def submit(self, rows):
        self.batches.append([(job.key, fi, box, start) for job, fi, box, start in rows])
        return [np.asarray(job.frames[fi]).copy() for job, fi, _, _ in rows]

    def result(self, item):
        return item


@pytest.fixture
def stub(monkeypatch):
    from wav2lip_amd import multiclip
    StubRunner.instances = []
    monkeypatch.setattr(multiclip, "BatchRunner", StubRunner)
    return multiclip


def _job(multiclip, key, n_rows, shape=(12, 10), n_frames=None):
    n_frames = n_frames or max(n_rows, 1)
    frames = np.zeros((n_frames,) + shape + (3,), np.uint8)
    for k in range(n_frames):
        frames[k, 0, 0] = (hash(key) % 251, k % 256, k // 256)
    mel = types.SimpleNamespace(shape=(80, 16 + 4 * n_rows))
    return multiclip.ClipJob(key, frames, mel, [(k, (1, 9, 2, 8), 3 * k) for k in range(n_rows)])


def test_batches_are_packed_across_jobs_and_order_is_kept(stub):
    lengths = [37, 61, 9, 50]
    events = []
    out = stub.lipsync_many(None, [_job(stub, "k%d" % i, n) for i, n in enumerate(lengths)], batch_size=32, depth=2,
                            sink=lambda key, f: events.append((key, None if f is None else tuple(int(v) for v in f[0, 0]))))
    assert out is None
    r = StubRunner.instances[-1]
    assert [len(b) for b in r.batches] == [32, 32, 32, 32, 29]
    flat = [row for b in r.batches for row in b]
    assert [(k, fi) for k, fi, _, _ in flat] == [("k%d" % i, j) for i, n in enumerate(lengths) for j in range(n)]
    assert [len({k for k, _, _, _ in b}) for b in r.batches] == [1, 2, 1, 3, 1]   # batches cross job boundaries
    want = []
    for i, n in enumerate(lengths):
        want += [("k%d" % i, (hash("k%d" % i) % 251, j % 256, j // 256)) for j in range(n)] + [("k%d" % i, None)]
    assert events == want
    got = stub.lipsync_many(None, [_job(stub, "a", 3), _job(stub, "b", 2, shape=(10, 20))], batch_size=4)
    assert sorted(got) == ["a", "b"] and [len(got[k]) for k in ("a", "b")] == [3, 2] and got["b"][0].shape == (10, 20, 3)
    assert StubRunner.instances[-1].args == (4, 4, "f32")                      # LIPSYNC_DEPTH lanes by default


def test_jobs_are_consumed_lazily_and_released_after_their_last_row(stub):
    import gc
    import weakref
    depth, bs, per_job, n_jobs = 2, 8, 4, 40
    refs, produced, peak = [], [0], [0]

    def jobs():
        for i in range(n_jobs):
            j = _job(stub, i, per_job)
            refs.append(weakref.ref(j.frames))
            produced[0] += 1
            yield j
            del j

    def sink(key, frame):
        gc.collect()
        alive = sum(r() is not None for r in refs)
        peak[0] = max(peak[0], alive)
        if frame is None:
            assert produced[0] - (key + 1) <= (depth + 1) * bs // per_job + 1   # the producer is not run ahead

    stub.lipsync_many(None, jobs(), batch_size=bs, depth=depth, sink=sink)
    assert produced[0] == n_jobs
    assert peak[0] <= (depth + 1) * bs // per_job + 1, peak[0]                  # jobs alive: those of depth + 1 batches, plus one
    gc.collect()
    assert all(r() is None for r in refs)


def test_zero_jobs_and_zero_row_jobs(stub):
    assert stub.lipsync_many(None, []) == {}
    events = []
    stub.lipsync_many(None, [_job(stub, "e0", 0), _job(stub, "a", 5), _job(stub, "e1", 0), _job(stub, "b", 2), _job(stub, "e2", 0)],
                      batch_size=4, depth=2, sink=lambda k, f: events.append((k, f is None)))
    closes = [k for k, c in events if c]
    assert closes == ["e0", "a", "e1", "b", "e2"]
    assert [k for k, c in events if not c] == ["a"] * 5 + ["b"] * 2
    assert stub.lipsync_many(None, [_job(stub, "only", 0)]) == {"only": []}


def test_a_box_outside_its_frame_names_the_job(stub):
    bad = _job(stub, "clip-17", 3)
    bad.rows[1] = (1, (1, 13, 2, 8), 3)                                       # y2 = 13 > H = 12
    with pytest.raises(ValueError, match="clip-17"):
        stub.lipsync_many(None, [_job(stub, "fine", 2), bad], batch_size=4)
    late = _job(stub, "clip-18", 2)
    late.rows[0] = (0, (1, 9, 2, 8), 100)                                     # mel window beyond the spectrogram
    with pytest.raises(ValueError, match="clip-18"):
        stub.lipsync_many(None, [late], batch_size=4)
    with pytest.raises(ValueError, match="clip-19"):
        stub.lipsync_many(None, [stub.ClipJob("clip-19", late.frames, late.mel, [(7, (1, 9, 2, 8), 0)])], batch_size=4)


def _surface(parser):
    rows = []
    for a in parser._actions:
        if a.dest == "help":
            continue
        rows.append([list(a.option_strings), a.dest, getattr(a.type, "__name__", None), a.default, a.nargs, bool(a.required),
                     type(a).__name__])
    return rows


def test_cli_surface_is_the_references_plus_the_two_precision_flags():
    from wav2lip_amd import gen_videos_from_filelist as gv
    ref = json.loads(str(G["cli"]))
    assert _surface(gv.parser) == ref
    assert [r[1] for r in ref] == ["filelist", "results_dir", "data_root", "checkpoint_path", "pads", "face_det_batch_size",
                                   "wav2lip_batch_size"]
    cli = _surface(gv.cli_parser)
    assert cli[:len(ref)] == ref and [r[1] for r in cli[len(ref):]] == ["precision", "face_det_precision"]
    a = gv.cli_parser.parse_args(["--filelist", "f", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"])
    assert (a.pads, a.face_det_batch_size, a.wav2lip_batch_size, a.precision, a.face_det_precision) == ([0, 0, 0, 0], 64, 128, "fp32", "fp32")


def test_lines_are_dealt_to_ranks_round_robin():
    from wav2lip_amd import gen_videos_from_filelist as gv
    lines = ["a%d v%d\n" % (i, i) for i in range(7)]
    parts = [gv.lines_of_rank(lines, types.SimpleNamespace(rank=r, world=3)) for r in range(3)]
    assert [[i for i, _ in p] for p in parts] == [[0, 3, 6], [1, 4], [2, 5]]
    assert sorted(x for p in parts for x in p) == list(enumerate(lines))       # every line once, with its own index
    assert gv.lines_of_rank(lines, types.SimpleNamespace(rank=0, world=1)) == list(enumerate(lines))
