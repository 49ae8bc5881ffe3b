"""Packed face detection on the device: w2l_s3fd_pack_rows(_bf16) byte for byte against the frame-batch pack kernels,
w2l_face_boxes_segments against the host statement of `face_detect`'s finish, `face_detection.detect_many` against a replay of
its own batches and against the executed reference (tests/golden/golden_filelist_v1.npz), and the two commands with
`--packed_face_det`."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_filelist_v1.npz"))
NO_FACE = 'Face not detected! Ensure the video contains a face in all the frames.'


# ---------------------------------------------------------------- w2l_s3fd_pack_rows / _bf16
def _stored_frames(cuda, n, H, W, seed):
    """n u8 [H,W,3] frames packed back to back in one allocation: 5x7 frames are 105 bytes, so they sit on addresses that are
    4-byte aligned, odd, even-but-not-aligned, odd in turn"""
    r = np.random.default_rng(seed)
    host = r.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    store = torch.from_numpy(host).to(cuda)
    assert store.data_ptr() % 16 == 0
    return store


@pytest.mark.parametrize("H,W,order", [(5, 7, [1, 0, 1]), (5, 7, [2, 3, 2]), (16, 16, [2, 0, 2])])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_pack_rows_equals_the_pack_kernel_on_the_gathered_frames(cuda, H, W, order, precision):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    store = _stored_frames(cuda, 4, H, W, seed=H)
    fb = H * W * 3
    addrs = [store.data_ptr() + i * fb for i in order]
    if H == 5:
        assert {a % 4 for a in addrs} == ({1, 0} if order[0] == 1 else {2, 3})      # the byte path and the dword path
    else:
        assert all(a % 4 == 0 for a in addrs)
    table = torch.from_numpy(np.asarray(addrs, dtype=np.uint64).view(np.int64)).to(cuda)
    gathered = store[order].contiguous()
    B = len(order)
    if precision == "f32":
        y = torch.full((B, H, W, 4), float("nan"), device=cuda)
        want = torch.full((B, H, W, 4), float("nan"), device=cuda)
        check(lib.w2l_s3fd_pack_rows(current_stream(), B, H, W, ptr(table), ptr(y), 4), "s3fd_pack_rows")
        check(lib.w2l_s3fd_pack(current_stream(), B * H * W, ptr(gathered), ptr(want), 4), "s3fd_pack")
        ref = gathered.cpu().numpy()[..., ::-1].astype(np.float32) - np.array([104, 117, 123], np.float32)
        assert np.array_equal(want.cpu().numpy()[..., :3], ref) and not want.cpu().numpy()[..., 3].any()
    else:
        y = torch.full((B, H, W, 8), float("nan"), device=cuda, dtype=torch.bfloat16)
        want = torch.full((B, H, W, 8), float("nan"), device=cuda, dtype=torch.bfloat16)
        check(lib.w2l_s3fd_pack_rows_bf16(current_stream(), B, H, W, ptr(table), ptr(y), 8), "s3fd_pack_rows_bf16")
        check(lib.w2l_s3fd_pack_bf16(current_stream(), B * H * W, ptr(gathered), ptr(want), 8), "s3fd_pack_bf16")
    assert not bool(torch.isnan(y.float()).any())                                 # every element written, pad channels included
    assert torch.equal(y, want)


def test_pack_rows_reports_argument_errors(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    store = _stored_frames(cuda, 2, 16, 16, seed=1)
    table = torch.zeros(4, dtype=torch.int64, device=cuda)
    table[:2] = torch.tensor([store.data_ptr(), store.data_ptr() + 768])
    y = torch.full((2, 16, 16, 8), 7., device=cuda)
    yb = torch.full((2, 16, 16, 8), 7., device=cuda, dtype=torch.bfloat16)
    s = current_stream()
    for B, Hh, t, out, cs in ((0, 16, table, y, 4), (2, 0, table, y, 4), (2, 16, None, y, 4), (2, 16, table, None, 4),
                              (2, 16, table, y, 2), (70000, 16, table, y, 4)):
        assert lib.w2l_s3fd_pack_rows(s, B, Hh, 16, ptr(t) if t is not None else None, ptr(out) if out is not None else None, cs) != 0
        assert b"s3fd_pack_rows" in lib.w2l_last_error()
    assert lib.w2l_s3fd_pack_rows(s, 2, 16, 16, table.data_ptr() + 4, ptr(y), 4) != 0 and b"8-byte" in lib.w2l_last_error()
    assert lib.w2l_s3fd_pack_rows(s, 2, 16, 16, ptr(table), y.data_ptr() + 4, 4) != 0 and b"16-byte" in lib.w2l_last_error()
    for B, t, out, cs in ((0, table, yb, 8), (2, None, yb, 8), (2, table, yb, 4), (2, table, yb, 12)):
        assert lib.w2l_s3fd_pack_rows_bf16(s, B, 16, 16, ptr(t) if t is not None else None, ptr(out), cs) != 0
        assert b"s3fd_pack_rows_bf16" in lib.w2l_last_error()
    assert lib.w2l_s3fd_pack_rows_bf16(s, 2, 16, 16, table.data_ptr() + 4, ptr(yb), 8) != 0
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((yb == 7).all())                         # nothing ran


# ---------------------------------------------------------------- w2l_face_boxes_segments
FH, FW = 40, 50
FENCE = 1000000
SENTINEL = -7


def _segments_case(cuda, lengths, seed, flag_edits=()):
    """segments side by side with one fence row of huge coordinates before, between and after them; rect coordinates in 0..70
    reach beyond the 40 x 50 frame.  Returns (segment table on the device, rects, flags, the host copies, [(row0, n)])"""
    from wav2lip_amd.face_detection import many
    from wav2lip_amd.face_detection.s3fd import RECT_FOUND
    r = np.random.default_rng(seed)
    R = sum(lengths) + len(lengths) + 1
    rects = np.full((R, 4), FENCE, np.int32)
    flags = np.full((R,), RECT_FOUND, np.int32)
    segs, row = [], 1
    for n in lengths:
        rects[row:row + n] = r.integers(0, 71, (n, 4))
        segs.append((row, n))
        row += n + 1
    for k, i, f in flag_edits:
        flags[segs[k][0] + i] = f
    t = np.zeros(len(segs), many.BOX_SEGMENT)
    for k, (row0, n) in enumerate(segs):
        t[k] = (row0, n, FH, FW)
    return torch.from_numpy(t.view(np.uint8)).to(cuda), torch.from_numpy(rects).to(cuda), torch.from_numpy(flags).to(cuda), rects, segs


def _run_segments(cuda, t_dev, rects, flags, n_seg, pads, T):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    boxes = torch.full((rects.shape[0], 4), SENTINEL, dtype=torch.int32, device=cuda)
    status = torch.full((n_seg, 2), SENTINEL, dtype=torch.int32, device=cuda)
    check(_lib.load().w2l_face_boxes_segments(current_stream(), n_seg, ptr(t_dev), ptr(rects), ptr(flags), *pads, T, ptr(boxes),
                                              ptr(status)), "face_boxes_segments")
    return boxes.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("T", [0, 1, 5])
@pytest.mark.parametrize("pads", [(0, 10, 0, 0), (3, 10, 5, 7), (-2, -10, -4, -3)])
def test_face_boxes_segments_is_the_host_expression(cuda, T, pads):
    """n = 1..4 are shorter than the window of 5 (the wrapped negative start, clipped at 0 for n = 1, 2), 5 and 6 sit on its edge,
    63, 64 and 65 on the edge of the kernel's chunk of 64 frames, 70 and 130 are two and three chunks, 200 is past the three
    chunks its ring holds.  Integer arithmetic and one correctly rounded fp64 division on both sides: equality is the bar."""
    from wav2lip_amd.face_detection import many
    lengths = [1, 2, 3, 4, 5, 6, 11, 63, 64, 65, 70, 130, 200]
    t_dev, rects, flags, rects_h, segs = _segments_case(cuda, lengths, seed=100 + 10 * T + pads[0])
    boxes, status = _run_segments(cuda, t_dev, rects, flags, len(segs), pads, T)
    assert not status.any()
    inside = np.zeros(len(rects_h), bool)
    for row0, n in segs:
        want = many.host_boxes(rects_h[row0:row0 + n].tolist(), FH, FW, pads, T)
        assert np.array_equal(boxes[row0:row0 + n], want), (n, boxes[row0:row0 + n], want)
        assert np.abs(boxes[row0:row0 + n]).max() < 1000                          # no fence row was read
        inside[row0:row0 + n] = True
    assert (boxes[~inside] == SENTINEL).all()                                     # no fence row was written


def test_face_boxes_segments_reports_no_face_and_host_rows_per_segment(cuda):
    from wav2lip_amd.face_detection import many
    from wav2lip_amd.face_detection.s3fd import RECT_HOST, RECT_NONE
    lengths = [6, 70, 9, 3, 5, 200]
    edits = [(1, 66, RECT_NONE), (1, 68, RECT_NONE), (2, 2, RECT_NONE), (2, 7, RECT_HOST), (2, 8, RECT_HOST), (3, 0, RECT_HOST),
             (5, 195, RECT_NONE)]
    t_dev, rects, flags, rects_h, segs = _segments_case(cuda, lengths, seed=3, flag_edits=edits)
    boxes, status = _run_segments(cuda, t_dev, rects, flags, len(segs), (0, 10, 0, 0), 5)
    # a RECT_NONE at row k: (1, k), the first one; a RECT_HOST after an earlier RECT_NONE still wins: (2, its row)
    assert status.tolist() == [[0, 0], [1, 66], [2, 7], [2, 0], [0, 0], [1, 195]]
    for k, (row0, n) in enumerate(segs):
        if status[k, 0]:
            assert not boxes[row0:row0 + n].any()
        else:                                                                     # the neighbours are untouched by it
            assert np.array_equal(boxes[row0:row0 + n], many.host_boxes(rects_h[row0:row0 + n].tolist(), FH, FW, (0, 10, 0, 0), 5))
        assert (boxes[row0 - 1] == SENTINEL).all() and (boxes[row0 + n] == SENTINEL).all()


def test_face_boxes_segments_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    t_dev, rects, flags, _, segs = _segments_case(cuda, [4], seed=1)
    boxes = torch.full((rects.shape[0], 4), SENTINEL, dtype=torch.int32, device=cuda)
    status = torch.full((1, 2), SENTINEL, dtype=torch.int32, device=cuda)
    s = current_stream()
    for n_seg, T in ((0, 5), (-1, 5), (1, -1), (1, 65)):
        assert lib.w2l_face_boxes_segments(s, n_seg, ptr(t_dev), ptr(rects), ptr(flags), 0, 0, 0, 0, T, ptr(boxes), ptr(status)) != 0
        assert b"face_boxes_segments" in lib.w2l_last_error()
    args = [ptr(t_dev), ptr(rects), ptr(flags), ptr(boxes), ptr(status)]
    for k in range(5):
        a = list(args)
        a[k] = None
        assert lib.w2l_face_boxes_segments(s, 1, a[0], a[1], a[2], 0, 0, 0, 0, 5, a[3], a[4]) != 0
    torch.cuda.synchronize()
    assert bool((boxes == SENTINEL).all()) and bool((status == SENTINEL).all())   # nothing ran
    assert lib.w2l_face_boxes_segments(s, 1, ptr(t_dev), ptr(rects), ptr(flags), 0, 0, 0, 0, 64, ptr(boxes), ptr(status)) == 0
    assert status.cpu().tolist() == [[0, 0]]


# ---------------------------------------------------------------- face_detection.detect_many
BS = 8
PADS = (0, 0, 0, 0)                  # what tests/golden/make_golden_filelist.py recorded with (the reference's default), T = 5


def _filelist_jobs():
    """(line index, frames [n,H,W,3]) of the lines of synthetic.FILELIST_LINES that reach detection: the frames the filelist
    command hands to face_detect (the video truncated to the chunk count of the line's audio)"""
    clips = synth.filelist_clips()
    chunks = {name: c for name, _, _, c, _ in synth.FILELIST_CLIPS}
    jobs = []
    for idx, (a, v) in enumerate(synth.FILELIST_LINES):
        frames = clips[v][0]
        if len(frames) >= chunks[a]:
            jobs.append((idx, frames[:chunks[a]]))
    return jobs


def _same(a, b):
    assert [r[0] for r in a] == [r[0] for r in b]
    for (_, xb, xe), (_, yb, ye) in zip(a, b):
        assert xe == ye and (xb is None) == (yb is None)
        if xb is not None:
            assert xb.dtype == yb.dtype and xb.tobytes() == yb.tobytes()


_RUNS = {}


def _packed_run(cuda, precision):
    """the filelist's clips through detect_many three times on one detector (device frames with the batches recorded, the same
    again, host frames); one run per precision for the whole module"""
    import importlib
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection import many
    s3fd = importlib.import_module("wav2lip_amd.face_detection.s3fd")         # `face_detection.s3fd` is the class
    if precision in _RUNS:
        return _RUNS[precision]
    det = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(cuda),
                                       state_dict=synth.s3fd_state_dict(), precision=precision)
    jobs = _filelist_jobs()
    dev_frames = [(idx, torch.from_numpy(np.ascontiguousarray(f)).to(cuda)) for idx, f in jobs]
    built, batches = [], []
    real = {"_Graph": s3fd._Graph, "batch": many._detect_batch}

    def counting(*a, **k):
        assert (a[5:] + (k.get("precision", "f32"),))[0] == precision            # every graph of the run is one of its precision
        built.append(a[1:4])
        return real["_Graph"](*a, **k)

    def recording(detector, frames, B, H, W, rects, flags, offset):
        batches.append((frames.cpu().numpy().view("<u8").copy(), B, H, W, offset))
        return real["batch"](detector, frames, B, H, W, rects, flags, offset)

    def run(items):
        return list(face_detection.detect_many(det, (face_detection.DetectJob(i, f) for i, f in items), pads=PADS, T=5, batch_size=BS))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(s3fd, "_Graph", counting)
        mp.setattr(many, "_detect_batch", recording)
        first = run(dev_frames)
    again = run(dev_frames)
    host = run([(idx, list(f)) for idx, f in jobs])
    _RUNS[precision] = dict(det=det, precision=precision, jobs=jobs, dev_frames=dev_frames, built=built, batches=batches,
                            first=first, again=again, host=host)
    return _RUNS[precision]


@pytest.fixture(scope="module", params=["f32", "bf16"])
def packed(request, cuda):
    return _packed_run(cuda, request.param)


def test_detect_many_builds_one_graph_per_run_of_a_shape_and_repeats_itself(cuda, packed):
    shapes = [f.shape[1:3] for _, f in packed["jobs"]]
    runs = [s for k, s in enumerate(shapes) if k == 0 or s != shapes[k - 1]]
    assert [tuple(b) for b in packed["built"]] == [(BS,) + tuple(s) for s in runs] and len(runs) == 3
    assert all(b[1] == BS for b in packed["batches"])
    assert [r[0] for r in packed["first"]] == [idx for idx, _ in packed["jobs"]] == [0, 1, 2, 3, 5]
    _same(packed["first"], packed["again"])                                       # two runs give the same bytes
    _same(packed["first"], packed["host"])                                        # host frames and device frames too


def test_detect_many_names_the_clip_without_a_face_and_leaves_its_neighbours_alone(cuda, packed):
    by_idx = {r[0]: r for r in packed["first"]}
    assert by_idx[1][1] is None and by_idx[1][2] == NO_FACE
    for idx, frames in packed["jobs"]:
        if idx != 1:
            assert by_idx[idx][2] is None and by_idx[idx][1].shape == (len(frames), 4)


def test_detect_many_equals_a_replay_of_its_batches(cuda, packed):
    """every recorded address is frame i of one of the device tensors: stack each batch's frames, run get_detections_for_batch on
    them (same B, so the same launches), lay the rects out as the arena rows and apply the host finish per clip"""
    from wav2lip_amd.face_detection import many
    where = {}
    for idx, t in packed["dev_frames"]:
        fb = t.shape[1] * t.shape[2] * 3
        for i in range(t.shape[0]):
            where[t.data_ptr() + i * fb] = (idx, i)
    tensors = dict(packed["dev_frames"])
    rows = []                                                                     # (line, frame, rect) per arena row, padding dropped
    expect = [(idx, i) for idx, t in packed["dev_frames"] for i in range(t.shape[0])]
    for addr, B, H, W, offset in packed["batches"]:
        if offset == 0:
            group_rows = []
            rows.append(group_rows)
        owners = [where[int(a)] for a in addr]
        stacked = torch.stack([tensors[idx][i] for idx, i in owners])
        assert tuple(stacked.shape) == (B, H, W, 3)
        group_rows += list(zip(owners, packed["det"].get_detections_for_batch(stacked)))
    flat = []
    for group_rows in rows:                                                       # a group's padding repeats its last row
        n = len(group_rows)
        while n > 1 and group_rows[n - 1][0] == group_rows[n - 2][0]:
            n -= 1
        flat += group_rows[:n]
    assert [o for o, _ in flat] == expect
    pos = 0
    for (idx, t), got in zip(packed["dev_frames"], packed["first"]):
        rects = [r for _, r in flat[pos:pos + t.shape[0]]]
        pos += t.shape[0]
        if any(r is None for r in rects):
            assert got[1] is None and idx == 1 and rects.index(None) == 7
            continue
        want = many.host_boxes(rects, t.shape[1], t.shape[2], PADS, 5)
        assert np.array_equal(got[1], want), (idx, np.abs(got[1] - want).max())


def test_detect_many_fp32_boxes_are_the_references(cuda):
    """boxes_<idx> of the golden file come from the executed reference on the CPU, at the pads recorded there; a mismatch would
    be a finding about batch composition (EXPERIMENTS.md), since the per-clip path has to match the same file"""
    for idx, boxes, error in _packed_run(cuda, "f32")["first"]:
        if int(G["written"][idx]):
            want = G["boxes_%d" % idx]
            differ = int((boxes != want).any(axis=1).sum())
            print("line %d: %d of %d boxes differ from the reference" % (idx, differ, len(want)))
            assert error is None and np.array_equal(boxes, want), (idx, differ)
        else:
            assert boxes is None and error == NO_FACE


# ---------------------------------------------------------------- the commands with --packed_face_det
def _gen_state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    from wav2lip_amd import container
    tmp = tmp_path_factory.mktemp("packed_det")
    data = str(tmp / "data")
    os.makedirs(data)
    clips = synth.filelist_clips()
    for name, (frames, pcm) in clips.items():
        container.write_avi(os.path.join(data, name + ".avi"), frames, 25, audio=pcm, audio_sr=16000)
    return tmp, data, clips


def test_filelist_command_with_packed_detection_writes_what_the_reference_wrote(cuda, data_dir):
    """the bars of test_multiclip_gpu.py's command tests, with --packed_face_det"""
    from wav2lip_amd import container, gen_videos_from_filelist as gv
    tmp, data, clips = data_dir
    results = str(tmp / "results")
    with open(str(tmp / "list.txt"), "w") as fh:
        fh.write("".join("%s %s\n" % l for l in synth.FILELIST_LINES))
    torch.save({"state_dict": {"module." + k: v for k, v in _gen_state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp / "ckpt.pth"))
    err = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("WORLD_SIZE", raising=False)
        with contextlib.redirect_stderr(err):
            written = gv.main(["--filelist", str(tmp / "list.txt"), "--results_dir", results, "--data_root", data, "--checkpoint_path",
                               str(tmp / "ckpt.pth"), "--wav2lip_batch_size", str(int(G["batch_size"])), "--face_det_batch_size", "16",
                               "--packed_face_det"], state_dict=synth.s3fd_state_dict())
    want = [i for i, w in enumerate(G["written"]) if w]
    assert written == want and sorted(os.listdir(results)) == sorted("%d.avi" % i for i in want)
    lines = [l for l in err.getvalue().splitlines() if "skipped" in l]
    assert len(lines) == 2 and lines[0].startswith("line 1 (c4 c4): skipped") and "Face not detected" in lines[0]     # in line order
    assert lines[1].startswith("line 4 (c5 c5): skipped") and "fewer frames (10) than mel chunks (20)" in lines[1]
    for idx, (a, v) in enumerate(synth.FILELIST_LINES):
        if not int(G["written"][idx]):
            continue
        clip = container.read_avi(os.path.join(results, "%d.avi" % idx))
        frames = clip["frames"]
        n = int(G["n_frames"][idx])
        assert len(frames) == n and clip["fps"] == 25.0 and clip["audio_sr"] == 16000
        assert np.array_equal(clip["audio"], clips[a][1])
        means = frames.reshape(n, -1).astype(np.float64).mean(axis=1)
        assert float(np.abs(means - G["mean_%d" % idx]).max()) <= 1e-2
        for r in G["rows_%d" % idx].tolist():
            y1, y2, x1, x2 = G["boxes_%d" % idx][r].tolist()
            ref = clips[v][0][r].copy()
            ref[y1:y2, x1:x2] = G["face_%d_%d" % (idx, r)]
            d = np.abs(frames[r].astype(np.int32) - ref.astype(np.int32))
            assert int(d.max()) <= 2 and float((d != 0).mean()) <= 2e-3, (idx, r, int(d.max()), float((d != 0).mean()))


def test_scores_command_with_packed_detection_scores_and_skips_the_same_clips(cuda, data_dir):
    """the directory of the filelist's clips, faces from the detector, with and without --packed_face_det: the same clips scored
    and skipped with the same messages, scores within the bar of test_lse_many_agrees_with_lse_like_per_clip (1e-3)"""
    from wav2lip_amd import calculate_scores as cs, models
    tmp, data, _ = data_dir
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.SyncNet_color().state_dict().items()}, seed=2)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer": None, "global_step": 1, "global_epoch": 0},
               str(tmp / "sync.pth"))
    runs = []
    for extra in ([], ["--packed_face_det"]):
        out, err = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            scored = cs.main(["--data_root", data, "--checkpoint_path", str(tmp / "sync.pth")] + extra, state_dict=synth.s3fd_state_dict())
        runs.append((scored, out.getvalue().splitlines(), err.getvalue()))
    (loop, loop_out, loop_err), (pk, pk_out, pk_err) = runs
    keys = [s["key"] for s in pk]
    assert keys == [s["key"] for s in loop] and keys == sorted(keys) and len(keys) >= 2
    assert "c4.avi" not in keys and "c2.avi" not in keys
    assert pk_err == loop_err and "c4.avi: skipped: Face not detected" in pk_err and "c2.avi: skipped: too short" in pk_err
    assert len(pk_out) == len(loop_out) == len(keys) + 2
    for a, b in zip(pk, loop):
        assert (a["n"], a["offset"]) == (b["n"], b["offset"])
        err = max(abs(a["lse_d"] - b["lse_d"]), abs(a["lse_c"] - b["lse_c"]))
        print("%s: packed vs per-clip detection, largest score difference %.3e" % (a["key"], err))
        assert err <= 1e-3
