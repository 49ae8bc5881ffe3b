"""ReSyncED generation on the device: w2l_resize_rows_u8 byte for byte against w2l_resize_u8 and oracle/resize_ref.py at the
smallest shapes where it can go wrong, device-resident clips in `multiclip.lipsync_many` against the same clips as host lists, and
`python -m wav2lip_amd.real_videos_inference` against the executed reference (tests/golden/golden_real_videos_v1.npz,
tests/golden/make_golden_real_videos.py)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import resize_ref
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_real_videos_v1.npz"))
FENCE, FENCE_BYTES = 0xA5, 64

# (Hs, Ws) -> (Hd, Wd)
COPY, AREA, ODD2X, DOWN, UP = ((6, 7), (6, 7)), ((8, 12), (4, 6)), ((7, 9), (3, 4)), ((11, 13), (7, 5)), ((5, 4), (9, 11))
WIDTHS = [((6, 9), (4, wd)) for wd in (1, 2, 3, 5, 8)]          # no full item, a ragged end, exactly two items
ONE_LINE = ((5, 9), (1, 6))


def _source(shape, seed):
    return np.random.default_rng([91, seed]).integers(0, 256, shape + (3,), dtype=np.uint8)


class Rows:
    """rows of ONE launch: every src and dst in a buffer of its own at a chosen byte offset, every dst between fences"""

    def __init__(self, cuda):
        self.cuda, self.rows, self.keep = cuda, [], []

    def source(self, arr, offset=0):
        buf = torch.zeros(offset + arr.size + 8, dtype=torch.uint8, device=self.cuda)
        buf[offset:offset + arr.size] = torch.from_numpy(arr.reshape(-1)).to(self.cuda)
        self.keep.append(buf)
        return buf.data_ptr() + offset

    def add(self, arr, dsize, src_offset=0, dst_offset=0, src_addr=None):
        Hd, Wd = dsize
        n = Hd * Wd * 3
        src_addr = self.source(arr, src_offset) if src_addr is None else src_addr
        dst = torch.full((FENCE_BYTES + dst_offset + n + FENCE_BYTES,), FENCE, dtype=torch.uint8, device=self.cuda)
        assert (src_addr - src_offset) % 4 == 0 and dst.data_ptr() % 4 == 0          # the offsets ARE the misalignments
        self.rows.append((arr, dsize, src_addr, dst, FENCE_BYTES + dst_offset))
        return src_addr

    def table(self):
        from wav2lip_amd import real_videos_inference as rv
        t = np.zeros(len(self.rows), rv.RESIZE_ROW)
        for i, (arr, (Hd, Wd), src_addr, dst, lo) in enumerate(self.rows):
            t[i] = (src_addr, dst.data_ptr() + lo, arr.shape[0], arr.shape[1], Hd, Wd)
        return torch.from_numpy(t.view(np.uint8)).to(self.cuda)

    def launch(self):
        from wav2lip_amd import _lib
        from wav2lip_amd._lib import check, current_stream, ptr
        table = self.table()
        mx = max(Hd * Wd for _, (Hd, Wd), _, _, _ in self.rows)
        check(_lib.load().w2l_resize_rows_u8(current_stream(), len(self.rows), ptr(table), mx), "resize_rows_u8")
        torch.cuda.synchronize()

    def check(self, want):
        """every row equals want(arr, dsize) and no byte outside any dst changed"""
        for i, (arr, (Hd, Wd), _, dst, lo) in enumerate(self.rows):
            got = dst.cpu().numpy()
            n = Hd * Wd * 3
            assert (got[:lo] == FENCE).all() and (got[lo + n:] == FENCE).all(), ("fence", i, arr.shape, (Hd, Wd))
            for name, ref in want(arr, (Hd, Wd)).items():
                assert np.array_equal(got[lo:lo + n].reshape(Hd, Wd, 3), ref), (name, i, arr.shape, (Hd, Wd), lo % 4)


_REF = {}


def _want(arr, dsize, cuda=None):
    """{"resize_u8": w2l_resize_u8 on that frame, "oracle": oracle/resize_ref.py}, computed once per (frame, size)"""
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    key = (arr.tobytes(), arr.shape, dsize)
    if key not in _REF:
        Hd, Wd = dsize
        dev = torch.device("cuda:0")
        src = torch.from_numpy(arr).to(dev)
        dst = torch.empty((1, Hd, Wd, 3), dtype=torch.uint8, device=dev)
        check(_lib.load().w2l_resize_u8(current_stream(), 1, ptr(src), arr.shape[0], arr.shape[1], ptr(dst), Hd, Wd), "resize_u8")
        _REF[key] = {"resize_u8": dst[0].cpu().numpy(), "oracle": resize_ref.resize_linear_u8(arr, (Wd, Hd))}
    return _REF[key]


def test_every_branch_and_every_line_width_in_one_launch_of_mixed_shapes(cuda):
    rows = Rows(cuda)
    cases = [COPY, AREA, ODD2X, DOWN, UP, ONE_LINE] + WIDTHS
    for k, (s, d) in enumerate(cases):
        rows.add(_source(s, k), d)
    assert len({(r[0].shape, r[1]) for r in rows.rows}) >= 3
    rows.launch()
    rows.check(_want)


@pytest.mark.parametrize("case", [AREA, DOWN, WIDTHS[4], WIDTHS[3], COPY], ids=["area", "down", "two_items", "ragged", "copy"])
def test_src_and_dst_at_every_byte_alignment(cuda, case):
    s, d = case
    rows = Rows(cuda)
    arr = _source(s, 40)
    for so in range(4):
        for do in range(4):
            rows.add(arr, d, src_offset=so, dst_offset=do)
    rows.launch()
    rows.check(_want)


def test_two_rows_share_one_source(cuda):
    rows = Rows(cuda)
    arr = _source((8, 12), 50)
    addr = rows.add(arr, (4, 6), src_offset=1)
    rows.add(arr, (4, 6), src_offset=1, dst_offset=3, src_addr=addr)          # a duplicated frame: the same bytes twice
    rows.add(arr, (5, 7), src_offset=1, src_addr=addr)                         # and the same source at another size
    rows.launch()
    rows.check(_want)
    a, b = (r[3].cpu().numpy()[r[4]:r[4] + 72] for r in rows.rows[:2])
    assert np.array_equal(a, b)


@pytest.mark.parametrize("B", [1, 70])
def test_one_row_and_more_rows_than_one_grid_row_of_items(cuda, B):
    rows = Rows(cuda)
    shapes = [DOWN, AREA, UP, WIDTHS[3]]
    for k in range(B):
        s, d = shapes[k % len(shapes)]
        rows.add(_source(s, 60 + k % 7), d, src_offset=k % 4, dst_offset=(k // 4) % 4)
    rows.launch()
    rows.check(_want)


def test_refusals_return_an_error_code_and_write_nothing(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    rows = Rows(cuda)
    rows.add(_source((11, 13), 70), (7, 5))
    table = rows.table()
    shifted = torch.zeros(table.numel() + 16, dtype=torch.uint8, device=cuda)
    shifted[8:8 + table.numel()] = table
    assert lib.w2l_resize_rows_u8(current_stream(), 1, None, 35) != 0
    assert lib.w2l_resize_rows_u8(current_stream(), 0, ptr(table), 35) != 0
    assert lib.w2l_resize_rows_u8(current_stream(), -1, ptr(table), 35) != 0
    assert lib.w2l_resize_rows_u8(current_stream(), 65536, ptr(table), 35) != 0
    assert lib.w2l_resize_rows_u8(current_stream(), 1, ptr(shifted[8:]), 35) != 0               # a misaligned table
    assert b"16-byte" in lib.w2l_last_error()
    assert lib.w2l_resize_rows_u8(current_stream(), 1, ptr(table), 0) != 0
    torch.cuda.synchronize()
    assert bool((rows.rows[0][3] == FENCE).all())                                                 # dst untouched
    assert lib.w2l_resize_rows_u8(current_stream(), 1, ptr(table), 35) == 0                      # and the same call, well formed
    torch.cuda.synchronize()
    rows.check(_want)


def test_the_python_entry_validates_the_sizes_the_kernel_cannot(cuda):
    from wav2lip_amd import real_videos_inference as rv
    src = torch.zeros((2, 6, 8, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="at least 1"):
        rv.resize_frames_device(src, (0, 4))
    with pytest.raises(ValueError, match="at least 1"):
        rv.resize_rows([(src.data_ptr(), src.data_ptr(), 6, 8, 40000, 40000)])
    arr = _source((11, 13), 80)
    both = torch.from_numpy(np.stack([arr, arr[::-1].copy()])).to(cuda)
    out = rv.resize_frames_device(both, (5, 7)).cpu().numpy()                 # 11*13*3 = 429 bytes: frame 1 starts at byte 429
    assert np.array_equal(out[0], _want(arr, (7, 5))["oracle"]) and np.array_equal(out[1], _want(arr[::-1].copy(), (7, 5))["oracle"])


# ---------------------------------------------------------------- device-resident clips
def _state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


@pytest.fixture(scope="module")
def model(cuda):
    from wav2lip_amd import models
    m = models.Wav2Lip()
    m.load_state_dict(_state_dict())
    return m.to(cuda).eval()


def test_device_resident_clips_give_the_bytes_of_host_clips(cuda, model):
    from wav2lip_amd import multiclip
    r = np.random.default_rng(33)
    host, resident = [], []
    for i, (n, (H, W)) in enumerate(((7, (40, 36)), (5, (33, 47)), (9, (40, 36)))):
        frames = r.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        mel = torch.from_numpy(r.uniform(-4, 4, (80, 16 + int((n - 1) * 3.2))).astype(np.float32)).to(cuda)
        boxes = [(2 + k % 3, H - 1 - k % 2, 1 + k % 4, W - 3 + k % 3) for k in range(n)]
        rows = multiclip.rows_filelist(mel.shape[1], n, boxes)
        rows[-1] = (0,) + rows[-1][1:]                                          # a frame named twice
        host.append(multiclip.ClipJob(i, list(frames), mel, rows))
        resident.append(multiclip.ClipJob(i, torch.from_numpy(frames).to(cuda), mel, rows))
    want = multiclip.lipsync_many(model, iter(host), batch_size=8)
    got = multiclip.lipsync_many(model, iter(resident), batch_size=8)
    again = multiclip.lipsync_many(model, iter(resident), batch_size=8)
    for j in host:
        assert len(want[j.key]) == len(got[j.key]) == len(j.rows) > 0
        for k, (a, b, c) in enumerate(zip(want[j.key], got[j.key], again[j.key])):
            assert np.array_equal(a, b) and np.array_equal(b, c), (j.key, k)
        assert not np.array_equal(got[j.key][0], j.frames[0])                   # something was pasted
    for j, jr in zip(host, resident):                                           # the resident frames are read, never written
        assert np.array_equal(jr.frames.cpu().numpy(), np.stack(j.frames))


# ---------------------------------------------------------------- the command
def _run_cli(tmp_path_factory, precision):
    from wav2lip_amd import container, real_videos_inference as rv
    assert torch.cuda.is_available()
    tmp = tmp_path_factory.mktemp("real_videos_" + precision)
    data, results = str(tmp / "data"), str(tmp / "results")
    os.makedirs(data)
    clips = synth.real_video_clips()
    for name, (frames, fps, pcm) in clips.items():
        container.write_avi(os.path.join(data, name + ".avi"), frames, fps, audio=pcm, audio_sr=16000)
    with open(str(tmp / "list.txt"), "w") as fh:
        fh.write("".join("%s %s\n" % l for l in synth.REAL_LINES))
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp / "ckpt.pth"))
    assert json.loads(str(G["flags"])) == synth.REAL_FLAGS
    mp = pytest.MonkeyPatch()
    mp.delenv("WORLD_SIZE", raising=False)
    err, report = io.StringIO(), {}
    with contextlib.redirect_stderr(err):
        written = rv.main(["--mode", "tts", "--filelist", str(tmp / "list.txt"), "--results_dir", results, "--data_root", data,
                           "--checkpoint_path", str(tmp / "ckpt.pth"), "--wav2lip_batch_size", str(int(G["batch_size"])),
                           "--precision", precision] + synth.REAL_FLAGS, state_dict=synth.s3fd_state_dict(), report=report)
    mp.undo()
    return dict(results=results, written=written, stderr=err.getvalue(), clips=clips, report=report)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    return _run_cli(tmp_path_factory, "fp32")


def test_cli_decides_what_the_reference_decided(cuda, cli_run):
    want = [i for i, w in enumerate(G["written"]) if w]
    assert cli_run["written"] == want
    assert sorted(os.listdir(cli_run["results"])) == sorted("%d.avi" % i for i in want)      # a gap where the clip was skipped
    assert "line 3 (r4 r4): skipped" in cli_run["stderr"] and "Face not detected" in cli_run["stderr"]
    rep = cli_run["report"]
    for i in range(len(synth.REAL_LINES)):
        assert rep[i]["read"] == tuple(G["size_read"][i].tolist()) and rep[i]["capped"] == tuple(G["size_capped"][i].tolist()), i
        if i not in want:
            assert "boxes" not in rep[i]
            continue
        assert rep[i]["factor"] == int(G["factor"][i]) and rep[i]["rescaled"] == tuple(G["size_final"][i].tolist()), i
        assert rep[i]["index"] == G["index_%d" % i].tolist(), i
        assert np.array_equal(rep[i]["boxes"], G["boxes_%d" % i]), (i, rep[i]["boxes"].tolist(), G["boxes_%d" % i].tolist())
    assert any(rep[i]["read"] != rep[i]["capped"] and rep[i]["factor"] > 1 for i in want)      # both resizes fired


def _rescaled_inputs(cli_run, idx):
    """the frames the generator pasted into, rebuilt on the host: oracle/resize_ref.py at the recorded sizes, by the index list"""
    src = cli_run["clips"][synth.REAL_LINES[idx][0]][0]
    (hr, wr), (hc, wc), (hf, wf) = (tuple(G[k][idx].tolist()) for k in ("size_read", "size_capped", "size_final"))
    out = {}
    for j in sorted(set(G["index_%d" % idx].tolist())):
        f = src[j]
        if (hc, wc) != (hr, wr):
            f = resize_ref.resize_linear_u8(f, (wc, hc))
        if (hf, wf) != (hc, wc):
            f = resize_ref.resize_linear_u8(f, (wf, hf))
        out[j] = f
    return out


def test_cli_frames_and_audio_match_the_reference(cuda, cli_run):
    """the comparison and the bars of tests/test_multiclip_gpu.py against golden_filelist_v1.npz: per-frame means within 1e-2,
    recorded rows within 2 levels on at most 2e-3 of the bytes"""
    from wav2lip_amd import container
    for idx, (v, a) in enumerate(synth.REAL_LINES):
        if not int(G["written"][idx]):
            continue
        clip = container.read_avi(os.path.join(cli_run["results"], "%d.avi" % idx))
        frames = clip["frames"]
        n = int(G["n_frames"][idx])
        assert len(frames) == n and abs(clip["fps"] - float(G["fps"][idx])) < 1e-9 and clip["audio_sr"] == 16000
        assert frames.shape[1:3] == tuple(G["size_final"][idx].tolist())
        assert np.array_equal(clip["audio"], cli_run["clips"][a][2])                    # the audio track: the source PCM
        src = _rescaled_inputs(cli_run, idx)
        index = G["index_%d" % idx].tolist()
        means = frames.reshape(n, -1).astype(np.float64).mean(axis=1)
        print("line %d: largest mean difference %.3e" % (idx, float(np.abs(means - G["mean_%d" % idx]).max())))
        assert float(np.abs(means - G["mean_%d" % idx]).max()) <= 1e-2
        for r in G["rows_%d" % idx].tolist():
            y1, y2, x1, x2 = G["boxes_%d" % idx][r].tolist()
            ref = src[index[r]].copy()
            ref[y1:y2, x1:x2] = G["face_%d_%d" % (idx, r)]
            d = np.abs(frames[r].astype(np.int32) - ref.astype(np.int32))
            print("line %d row %d: max %d, differing %.2e" % (idx, r, int(d.max()), float((d != 0).mean())))
            assert int(d.max()) <= 2 and float((d != 0).mean()) <= 2e-3, (idx, r, int(d.max()), float((d != 0).mean()))
            outside = frames[r].copy()
            outside[y1:y2, x1:x2] = ref[y1:y2, x1:x2]
            assert np.array_equal(outside, ref)                                         # outside the box: the resized frame, exactly


def test_cli_bf16_runs_and_writes_the_same_files(cuda, cli_run, tmp_path_factory):
    from wav2lip_amd import container
    run = _run_cli(tmp_path_factory, "bf16")
    assert run["written"] == cli_run["written"]
    assert sorted(os.listdir(run["results"])) == sorted(os.listdir(cli_run["results"]))
    for idx in run["written"]:
        a = container.read_avi(os.path.join(run["results"], "%d.avi" % idx))["frames"]
        assert a.shape == (int(G["n_frames"][idx]),) + tuple(G["size_final"][idx].tolist()) + (3,)
