"""Filelist generation on the device: the row-table kernels (w2l_crop_resize_rows_u8, w2l_compose_rows_u8, w2l_mel_gather_rows)
bit for bit against the one-video kernels they generalise, `multiclip.lipsync_many` against `Wav2LipRunner.run_frames` and the
oracle chain, and `python -m wav2lip_amd.gen_videos_from_filelist` against the executed reference
(tests/golden/golden_filelist_v1.npz, tests/golden/make_golden_filelist.py)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import datagen_ref, models_ref, resize_ref
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_filelist_v1.npz"))


def _state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


def _model(cuda):
    from wav2lip_amd import models
    m = models.Wav2Lip()
    m.load_state_dict(_state_dict())
    return m.to(cuda).eval()


def _table(cuda, dtype, entries):
    from wav2lip_amd import multiclip
    t = np.zeros(len(entries), dtype)
    for i, e in enumerate(entries):
        t[i] = e
    assert dtype in (multiclip.FRAME_ROW, multiclip.MEL_ROW)
    return torch.from_numpy(t.view(np.uint8)).to(cuda)


def _frame_rows(cuda, clips, rows, dst=None):
    """rows: (clip, frame, box); dst: one output tensor per row (None: in place)"""
    from wav2lip_amd import multiclip
    ent = []
    for r, (c, f, (y1, y2, x1, x2)) in enumerate(rows):
        fr = clips[c][f]
        ent.append((fr.data_ptr(), fr.data_ptr() if dst is None else dst[r].data_ptr(), fr.shape[0], fr.shape[1], y1, y2, x1, x2, (0, 0)))
    return _table(cuda, multiclip.FRAME_ROW, ent)


def _ref_crop(lib, cuda, clip, idx, boxes):
    from wav2lip_amd._lib import check, current_stream, ptr
    out = torch.empty((len(idx), 96, 96, 3), dtype=torch.uint8, device=cuda)
    b = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    i = torch.tensor(idx, dtype=torch.int32, device=cuda)
    check(lib.w2l_crop_resize_u8(current_stream(), len(idx), ptr(clip), clip.shape[1], clip.shape[2], ptr(i), ptr(b), 96, ptr(out)))
    return out


def _ref_paste(lib, cuda, clip, idx, boxes, pred):
    from wav2lip_amd._lib import check, current_stream, ptr
    b = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    out = clip.index_select(0, torch.tensor(idx, device=cuda))
    mx = max((y2 - y1) * (x2 - x1) for y1, y2, x1, x2 in boxes)
    check(lib.w2l_resize_paste_u8(current_stream(), len(idx), ptr(pred), 96, ptr(b), None, ptr(out), clip.shape[1], clip.shape[2], mx))
    return out


def _check_rows_case(cuda, clips, rows, in_place=False):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    n = len(rows)
    faces = torch.empty((n, 96, 96, 3), dtype=torch.uint8, device=cuda)
    pred = torch.from_numpy(synth.face_crops_u8(n, seed=5)).to(cuda)
    want_faces, want_out = [None] * n, [None] * n
    for c in sorted({r[0] for r in rows}):
        mine = [k for k, r in enumerate(rows) if r[0] == c]
        idx, boxes = [rows[k][1] for k in mine], [rows[k][2] for k in mine]
        wf = _ref_crop(lib, cuda, clips[c], idx, boxes)
        wo = _ref_paste(lib, cuda, clips[c], idx, boxes, pred[mine].contiguous())
        for j, k in enumerate(mine):
            want_faces[k], want_out[k] = wf[j], wo[j]
    work = [c.clone() for c in clips] if in_place else clips
    dst = None if in_place else [torch.full_like(clips[c][f], 7) for c, f, _ in rows]
    table = _frame_rows(cuda, work, rows, dst)
    check(lib.w2l_crop_resize_rows_u8(current_stream(), n, ptr(table), 96, ptr(faces)), "crop_resize_rows")
    mx = max(clips[c].shape[1] * clips[c].shape[2] for c, _, _ in rows)
    check(lib.w2l_compose_rows_u8(current_stream(), n, ptr(pred), 96, ptr(table), mx), "compose_rows")
    torch.cuda.synchronize()
    for k, (c, f, _) in enumerate(rows):
        assert torch.equal(faces[k], want_faces[k]), ("crop", k, rows[k])
        got = work[c][f] if in_place else dst[k]
        assert torch.equal(got, want_out[k]), ("compose", k, rows[k])
    if in_place:                                              # frames no row names are untouched
        named = {(c, f) for c, f, _ in rows}
        for c in range(len(clips)):
            for f in range(clips[c].shape[0]):
                if (c, f) not in named:
                    assert torch.equal(work[c][f], clips[c][f])


@pytest.fixture(scope="module")
def three_clips(cuda):
    r = np.random.default_rng(21)
    return [torch.from_numpy(r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)).to(cuda)
            for n, h, w in ((4, 120, 150), (3, 200, 210), (5, 97, 131))]


def test_row_kernels_equal_the_one_video_kernels_bit_for_bit(cuda, three_clips):
    mixed = [(0, 1, (10, 100, 20, 130)), (1, 0, (3, 99, 100, 196)), (2, 4, (0, 97, 0, 131)), (1, 2, (4, 196, 10, 202)),
             (0, 3, (0, 120, 0, 150)), (2, 0, (1, 96, 5, 60)), (0, 0, (24, 120, 54, 150)), (1, 1, (0, 37, 0, 41)),
             (2, 2, (50, 97, 100, 131)), (0, 2, (0, 96, 0, 96))]
    _check_rows_case(cuda, three_clips, mixed)                                        # three shapes in ONE launch
    _check_rows_case(cuda, three_clips, [(0, 0, (5, 101, 7, 103)), (1, 1, (100, 196, 0, 96))])            # identity: 96x96 boxes
    _check_rows_case(cuda, three_clips, [(1, 0, (0, 192, 0, 192)), (1, 2, (8, 200, 18, 210))])            # the 2x fast path
    _check_rows_case(cuda, three_clips, [(2, 1, (11, 80, 13, 121)), (0, 2, (30, 33, 40, 140))])           # generic
    _check_rows_case(cuda, three_clips, [(0, 0, (0, 120, 0, 150)), (2, 3, (0, 97, 0, 131)), (1, 0, (0, 200, 0, 50)),
                                         (1, 1, (150, 200, 160, 210))])                                  # all four edges
    _check_rows_case(cuda, three_clips, [(2, 2, (9, 90, 17, 100))])                                       # B = 1
    _check_rows_case(cuda, three_clips, [(0, 1, (10, 100, 20, 130)), (1, 0, (0, 192, 0, 192)), (2, 4, (0, 97, 0, 131)),
                                         (0, 3, (7, 103, 9, 105))], in_place=True)                      # src == dst


def test_row_kernels_report_argument_errors(cuda, three_clips):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    table = _frame_rows(cuda, three_clips, [(0, 0, (0, 96, 0, 96))])
    out = torch.empty((1, 96, 96, 3), dtype=torch.uint8, device=cuda)
    assert lib.w2l_crop_resize_rows_u8(current_stream(), 1, None, 96, ptr(out)) != 0
    assert lib.w2l_crop_resize_rows_u8(current_stream(), 0, ptr(table), 96, ptr(out)) != 0
    assert lib.w2l_crop_resize_rows_u8(current_stream(), 65536, ptr(table), 96, ptr(out)) != 0
    assert lib.w2l_compose_rows_u8(current_stream(), 1, ptr(out), 96, None, 100) != 0
    big = torch.zeros(64, dtype=torch.uint8, device=cuda)
    assert lib.w2l_compose_rows_u8(current_stream(), 1, ptr(out), 96, ptr(big[8:]), 100) != 0              # misaligned table
    assert lib.w2l_mel_gather_rows(current_stream(), ptr(big[8:]), 1, ptr(out), 4, 4) != 0
    assert b"16-byte" in lib.w2l_last_error()
    assert lib.w2l_mel_gather_rows_bf16(current_stream(), None, 1, ptr(out), 8, 8) != 0


def _mels(cuda, lengths, seed=2):
    r = np.random.default_rng(seed)
    return [torch.from_numpy(r.uniform(-4, 4, (80, t)).astype(np.float32)).to(cuda) for t in lengths]


def test_mel_gather_rows_equals_mel_gather_per_clip(cuda):
    from wav2lip_amd import _lib, multiclip
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    mels = _mels(cuda, (40, 133, 16))
    rows = [(0, 0), (1, 100), (0, 24), (2, 0), (1, 117), (1, 3), (0, 7)]
    table = _table(cuda, multiclip.MEL_ROW, [(mels[c].data_ptr(), mels[c].shape[1], s) for c, s in rows])
    n = len(rows)
    for name, dtype, cs in (("w2l_mel_gather", torch.float32, 4), ("w2l_mel_gather_bf16", torch.bfloat16, 8)):
        got = torch.full((n, 80, 16, cs), 9, dtype=dtype, device=cuda)
        rows_fn = getattr(lib, name.replace("gather", "gather_rows"))
        check(rows_fn(current_stream(), ptr(table), n, ptr(got), cs, cs), name)
        for c in range(3):
            mine = [k for k, r in enumerate(rows) if r[0] == c]
            st = torch.tensor([rows[k][1] for k in mine], dtype=torch.int32, device=cuda)
            want = torch.full((len(mine), 80, 16, cs), 9, dtype=dtype, device=cuda)
            check(getattr(lib, name)(current_stream(), ptr(mels[c]), mels[c].shape[1], ptr(st), len(mine), ptr(want), cs, cs), name)
            assert torch.equal(got[mine].view(torch.uint8), want.view(torch.uint8)), (name, c)


def _one_shape_jobs(cuda, lengths=(37, 20, 9), shape=(120, 150)):
    from wav2lip_amd import multiclip
    r = np.random.default_rng(31)
    jobs = []
    for i, n in enumerate(lengths):
        frames = r.integers(0, 256, (n + 2,) + shape + (3,), dtype=np.uint8)
        mel = _mels(cuda, (16 + int((n - 1) * 3.2) + 5,), seed=40 + i)[0]
        boxes = [(10 + k % 5, 100 + k % 7, 20 + k % 3, 130 - k % 4) for k in range(n + 2)]
        jobs.append(multiclip.ClipJob("clip%d" % i, frames, mel, multiclip.rows_filelist(mel.shape[1], n + 2, boxes)[:n]))
    return jobs


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_lipsync_many_equals_run_frames_on_the_concatenated_clips(cuda, precision):
    from wav2lip_amd import inference, multiclip
    model = _model(cuda)
    jobs = _one_shape_jobs(cuda)
    got = multiclip.lipsync_many(model, iter(jobs), batch_size=32, precision=precision)
    again = multiclip.lipsync_many(model, iter(jobs), batch_size=32, depth=2, precision=precision)
    frames, idx, boxes, mw = [], [], [], []
    for j in jobs:
        for fi, box, s in j.rows:
            frames.append(j.frames[fi])
            idx.append(len(idx))
            boxes.append(box)
            mw.append(j.mel[:, s:s + 16])
    frames_dev = torch.from_numpy(np.stack(frames)).to(cuda)
    mw = torch.stack(mw).contiguous()
    runner = inference.Wav2LipRunner(model, 32, **inference._precision_kw(precision))
    want = []
    for lo in range(0, len(idx), 32):
        hi = min(len(idx), lo + 32)
        want += list(runner.run_frames(frames_dev, idx[lo:hi], boxes[lo:hi], mel_windows=mw[lo:hi]).cpu().numpy())
    flat = [f for j in jobs for f in got[j.key]]
    assert [len(got[j.key]) for j in jobs] == [len(j.rows) for j in jobs] and len(flat) == len(want) == 66
    for k, (a, b) in enumerate(zip(flat, want)):
        assert np.array_equal(a, b), (precision, k, int(np.abs(a.astype(int) - b.astype(int)).max()))
    for j in jobs:                                              # a second run (another depth): the same bytes
        assert all(np.array_equal(a, b) for a, b in zip(got[j.key], again[j.key]))


def test_ragged_shapes_end_to_end_against_the_oracle_chain(cuda):
    """clips of three frame shapes in shared batches; sampled rows against resize_ref / datagen_ref / models_ref with the
    tolerance of test_golden_datapath_gpu.py (at most 2 levels, at most 2e-3 of the bytes); outside the box: the input"""
    from wav2lip_amd import multiclip
    model, sd = _model(cuda), _state_dict()
    r = np.random.default_rng(77)
    jobs = []
    for i, (n, shape) in enumerate(((21, (120, 150)), (30, (160, 160)), (5, (97, 131)), (17, (120, 150)))):
        frames = r.integers(0, 256, (n,) + shape + (3,), dtype=np.uint8)
        mel = _mels(cuda, (16 + int((n - 1) * 3.2),), seed=60 + i)[0]
        H, W = shape
        boxes = [(5 + k % 4, H - 9 - k % 3, 11 + k % 5, W - 20 + k % 2) for k in range(n)]
        jobs.append(multiclip.ClipJob(i, frames, mel, multiclip.rows_filelist(mel.shape[1], n, boxes)))
    got = multiclip.lipsync_many(model, jobs, batch_size=16)
    for j in jobs:
        assert len(got[j.key]) == len(j.rows)
        mel = j.mel.cpu().numpy()
        for k in sorted({0, len(j.rows) // 2, len(j.rows) - 1}):
            fi, box, s = j.rows[k]
            face = resize_ref.crop_resize(j.frames[fi], box)
            img, melb = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(face[None], mel[None, :, s:s + 16]))
            pred = datagen_ref.frames_to_u8(models_ref.wav2lip_forward(sd, torch.from_numpy(melb), torch.from_numpy(img)).numpy())
            ref = resize_ref.resize_paste(j.frames[fi].copy(), pred[0], box)
            d = np.abs(got[j.key][k].astype(np.int32) - ref.astype(np.int32))
            print("job %d row %d: max %d, differing %.2e" % (j.key, k, int(d.max()), float((d != 0).mean())))
            assert int(d.max()) <= 2 and float((d != 0).mean()) <= 2e-3, (j.key, k, int(d.max()), float((d != 0).mean()))
            outside = got[j.key][k].copy()
            y1, y2, x1, x2 = box
            outside[y1:y2, x1:x2] = j.frames[fi][y1:y2, x1:x2]
            assert np.array_equal(outside, j.frames[fi])


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from wav2lip_amd import container, gen_videos_from_filelist as gv
    assert torch.cuda.is_available()
    tmp = tmp_path_factory.mktemp("filelist")
    data, results = str(tmp / "data"), str(tmp / "results")
    os.makedirs(data)
    clips = synth.filelist_clips()
    for name, (frames, pcm) in clips.items():
        container.write_avi(os.path.join(data, name + ".avi"), frames, 25, audio=pcm, audio_sr=16000)
    with open(str(tmp / "list.txt"), "w") as fh:
        fh.write("".join("%s %s\n" % l for l in synth.FILELIST_LINES))
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp / "ckpt.pth"))
    mp = pytest.MonkeyPatch()
    mp.delenv("WORLD_SIZE", raising=False)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        written = gv.main(["--filelist", str(tmp / "list.txt"), "--results_dir", results, "--data_root", data, "--checkpoint_path",
                           str(tmp / "ckpt.pth"), "--wav2lip_batch_size", str(int(G["batch_size"]))], state_dict=synth.s3fd_state_dict())
    mp.undo()
    return dict(results=results, written=written, stderr=err.getvalue(), clips=clips)


def test_cli_writes_the_files_the_reference_wrote_and_skips_what_it_skipped(cuda, cli_run):
    want = [i for i, w in enumerate(G["written"]) if w]
    assert cli_run["written"] == want
    assert sorted(os.listdir(cli_run["results"])) == sorted("%d.avi" % i for i in want)
    err = cli_run["stderr"]
    assert "line 1 (c4 c4): skipped" in err and "Face not detected" in err
    assert "line 4 (c5 c5): skipped" in err and "fewer frames (10) than mel chunks (20)" in err


def test_cli_frames_and_audio_match_the_reference(cuda, cli_run):
    from wav2lip_amd import container
    for idx, (a, v) in enumerate(synth.FILELIST_LINES):
        if not int(G["written"][idx]):
            continue
        clip = container.read_avi(os.path.join(cli_run["results"], "%d.avi" % idx))
        frames = clip["frames"]
        n = int(G["n_frames"][idx])
        assert len(frames) == n and clip["fps"] == 25.0 and clip["audio_sr"] == 16000
        assert np.array_equal(clip["audio"], cli_run["clips"][a][1])                    # the audio track: the source PCM
        src = cli_run["clips"][v][0]
        means = frames.reshape(n, -1).astype(np.float64).mean(axis=1)
        print("line %d: largest mean difference %.3e" % (idx, float(np.abs(means - G["mean_%d" % idx]).max())))
        assert float(np.abs(means - G["mean_%d" % idx]).max()) <= 1e-2
        for r in G["rows_%d" % idx].tolist():
            y1, y2, x1, x2 = G["boxes_%d" % idx][r].tolist()
            ref = src[r].copy()
            ref[y1:y2, x1:x2] = G["face_%d_%d" % (idx, r)]
            d = np.abs(frames[r].astype(np.int32) - ref.astype(np.int32))
            print("line %d row %d: max %d, differing %.2e" % (idx, r, int(d.max()), float((d != 0).mean())))
            assert int(d.max()) <= 2 and float((d != 0).mean()) <= 2e-3, (idx, r, int(d.max()), float((d != 0).mean()))


def test_packed_run_holds_two_plans_per_lane_a_per_clip_loop_one_per_length(cuda, cli_run):
    from wav2lip_amd import inference, multiclip
    clips = cli_run["clips"]
    packed, loop = _model(cuda), _model(cuda)
    jobs, lengths = [], []
    for idx, (a, v) in enumerate(synth.FILELIST_LINES):
        if not int(G["written"][idx]):
            continue
        from wav2lip_amd import audio
        wav = clips[a][1][:, 0].astype(np.float32) / np.float32(32768.0)
        mel = audio.melspectrogram_device(wav, cuda)
        boxes = [tuple(b) for b in G["boxes_%d" % idx].tolist()]
        frames = list(clips[v][0][:len(boxes)])
        jobs.append(multiclip.ClipJob(idx, frames, mel, multiclip.rows_filelist(mel.shape[1], len(frames), boxes)))
        out = inference.lipsync(loop, frames, wav, box=boxes[0])
        lengths.append(len(out))
    multiclip.lipsync_many(packed, jobs, batch_size=128)
    sizes_packed = {k[0] for k in packed._graphs}
    per_lane = {}
    for k in packed._graphs:
        per_lane.setdefault(k[4], set()).add(k[0])
    sizes_loop = {k[0] for k in loop._graphs}
    print("plans: packed %d (batch sizes %s), per-clip loop %d (batch sizes %s)"
          % (len(packed._graphs), sorted(sizes_packed), len(loop._graphs), sorted(sizes_loop)))
    assert sizes_packed == {128, 157 - 128} and all(len(v) <= 2 for v in per_lane.values()) and len(packed._graphs) == 2
    assert sizes_loop == set(lengths) and len(set(lengths)) == 4 and len(loop._graphs) == 4
