"""Filelist scoring without a device: the window list of `evaluation.sync_rows` against the loop of oracle/lse_ref.py, the
packing of `evaluation.lse_many` (groups, batches, arena rows, padding, result order) with the two device steps stubbed and
host tensors standing in for device ones, and the flags of `python -m wav2lip_amd.calculate_scores`."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import lse_ref, models_ref


@pytest.mark.parametrize("fps", [25., 29.97, 30.])
def test_sync_rows_is_the_window_list_of_the_oracle_loop(monkeypatch, fps):
    """frame v is filled with v and mel column c with c, so the tensors the oracle's loop hands to its SyncNet name the windows"""
    from wav2lip_amd import evaluation
    seen = {}

    def capture(sd, mels, faces):
        seen["rows"] = [(int(round(float(f[0, 0, 0]) * 255)), int(m[0, 0, 0])) for f, m in zip(faces, mels)]
        return faces, mels

    monkeypatch.setattr(models_ref, "syncnet_forward", capture)
    monkeypatch.setattr(lse_ref, "scores", lambda v, a, vshift: None)
    for T in (4, 5, 6, 40):
        frames = np.broadcast_to(np.arange(T, dtype=np.uint8)[:, None, None, None], (T, 96, 96, 3))
        for Tm in (15, 16, 17, 80, 200):
            mel = np.broadcast_to(np.arange(Tm, dtype=np.float32)[None, :], (80, Tm))
            seen.clear()
            try:
                lse_ref.lse_like(None, frames, mel, fps=fps)
            except RuntimeError:                     # torch.stack of no windows
                seen["rows"] = []
            got = evaluation.sync_rows(T, Tm, fps)
            assert got == seen["rows"], (fps, T, Tm)
            assert len(got) == 0 or (got[0] == (0, 0) and got[-1][0] <= T - 5 and got[-1][1] + 16 <= Tm)
    assert evaluation.sync_rows(40, 200, 25.)[:3] == [(0, 0), (1, 3), (2, 6)]


class FakeSyncNet:
    """records every embed_rows call; a row's embeddings name its window: audio[0] = first byte of the window's first frame (read
    through the table's address, so staged host faces and faces that were tensors already are both followed), face[0] = start"""

    def __init__(self):
        self.training, self.calls, self.modes = True, [], []

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def embed_rows(self, rows, B, audio_out, face_out, offset=0):
        from wav2lip_amd import evaluation
        assert not self.training
        t = rows.numpy().view(evaluation.SYNC_ROW)
        assert len(t) == B and (t["pad"] == 0).all()
        first = np.array([ctypes.c_uint8.from_address(int(a)).value for a in t["frames"]], dtype=np.float32)
        audio_out[offset:offset + B] = 0
        face_out[offset:offset + B] = 0
        audio_out[offset:offset + B, 0] = torch.from_numpy(first)
        face_out[offset:offset + B, 0] = torch.from_numpy(t["start"].astype(np.float32))
        audio_out[offset:offset + B, 1] = torch.from_numpy(t["T"].astype(np.float32))
        self.calls.append((B, offset, tuple(audio_out.shape), t.copy()))


def _jobs(counts, pulled, host_every=2):
    """clip c: frames filled with 10 * (c % 20) + v % 10, a mel of its own length; every `host_every`-th clip's faces stay a host array"""
    from wav2lip_amd import evaluation
    for c, n in enumerate(counts):
        T = n + 4 if n else 3
        faces = np.empty((T, 96, 96, 3), np.uint8)
        faces[:] = (10 * (c % 20) + np.arange(T) % 10).astype(np.uint8)[:, None, None, None]
        mel = torch.zeros((80, 16 + int(3.2 * max(n - 1, 0)) + 1 + c % 2), dtype=torch.float32)
        assert len(evaluation.sync_rows(T, mel.shape[1], 25.)) == n
        pulled.append(c)
        yield evaluation.ScoreJob("clip%d" % c, faces if c % host_every == 0 else torch.from_numpy(faces), mel)


def test_lse_many_packs_windows_into_full_batches_and_keeps_job_order(monkeypatch):
    from wav2lip_amd import evaluation
    counts = [30, 0, 30, 10, 0, 7, 64, 3, 0]
    bs, vshift = 4, 2
    win = 2 * vshift + 1
    net, launches, pulled = FakeSyncNet(), [], []

    def fake_score(n_seg, segs, vs, face_emb, audio_emb, out):
        s = segs.numpy().view(evaluation.LSE_SEGMENT).copy()
        assert len(s) == n_seg and vs == vshift
        launches.append((s, face_emb.clone(), audio_emb.clone(), len(pulled), len(net.calls)))
        o = out.numpy()
        for k, (row0, n) in enumerate(s.tolist()):
            o[4 * k:4 * k + 4] = (float(audio_emb[row0, 0]), 0.25, k - 1, n)         # lse_d names the clip's first frame
            o[4 * n_seg + k * win:4 * n_seg + (k + 1) * win] = float(face_emb[row0 + n - 1, 0])   # mdist its last window's start

    monkeypatch.setattr(evaluation, "_score_segments", fake_score)
    res = evaluation.lse_many(net, _jobs(counts, pulled), vshift=vshift, batch_size=bs)
    assert net.training is True                                               # eval for the call, restored afterwards
    assert [r["key"] for r in res] == ["clip%d" % c for c in range(len(counts))]          # job order, n = 0 clips in their places
    assert [r["n"] for r in res] == counts
    for c, r in enumerate(res):
        if counts[c] == 0:
            assert r["offset"] is None and r["lse_c"] is None and r["lse_d"] is None and r["mdist"] is None
        else:
            assert r["lse_d"] == 10 * (c % 20) and r["lse_c"] == 0.25 and isinstance(r["offset"], int)
            assert r["mdist"].shape == (win,) and (r["mdist"] == int(80. * ((counts[c] - 1) / 25.))).all()
    # groups close between clips, as soon as 16 batches of windows are in: [30, 0, 30, 10] [0, 7, 64] [3, 0]
    groups = [[30, 30, 10], [7, 64], [3]]
    assert [l[0]["n"].tolist() for l in launches] == groups
    assert [l[3] for l in launches] == [4, 7, 9]                              # jobs read when each group ran: lazily consumed
    assert [r["offset"] for r in res if r["n"]] == [-1, 0, 1, -1, 0, -1]
    done = 0
    for segs, face_emb, audio_emb, _, ncalls in launches:
        W = int(segs["n"].sum())
        padded = -(-W // bs) * bs
        assert segs["row0"].tolist() == [0] + np.cumsum(segs["n"])[:-1].tolist()          # segments tile the arena without gaps
        calls = net.calls[done:ncalls]
        done = ncalls
        assert [c[0] for c in calls] == [bs] * (padded // bs)                # every batch has exactly batch_size rows
        assert [c[1] for c in calls] == list(range(0, padded, bs))
        assert all(c[2] == (padded, 512) for c in calls) and tuple(face_emb.shape) == (padded, 512)
        table = np.concatenate([c[3] for c in calls])
        for k in range(W, padded):                                            # padding repeats the last row, into the scratch tail
            assert table[k] == table[W - 1]
        # every arena row below W holds the window it should: clip's frame v and its start column
        for row0, n in segs.tolist():
            v = np.arange(n)
            assert (face_emb[row0:row0 + n, 0].numpy() == [int(80. * (x / 25.)) for x in v]).all()
            assert (audio_emb[row0:row0 + n, 0].numpy() % 10 == v % 10).all()
            assert len(set((audio_emb[row0:row0 + n, 0].numpy() // 10).tolist())) == 1
            assert len(set(audio_emb[row0:row0 + n, 1].tolist())) == 1       # one spectrogram per clip
    assert done == len(net.calls)


def test_lse_many_streams_results_to_a_sink_and_refuses_bad_jobs(monkeypatch):
    from wav2lip_amd import evaluation
    net, got = FakeSyncNet(), []
    net.training = False
    monkeypatch.setattr(evaluation, "_score_segments", lambda n_seg, segs, vs, f, a, out: out.zero_())
    assert evaluation.lse_many(net, _jobs([2, 0], []), vshift=1, batch_size=8, sink=got.append) is None
    assert [(r["key"], r["n"]) for r in got] == [("clip0", 0), ("clip1", 0)] and got[0]["mdist"].shape == (3,)   # the stub's n
    assert net.training is False and len(net.calls) == 1 and net.calls[0][:3] == (8, 0, (8, 512))
    assert evaluation.lse_many(net, iter(()), batch_size=8) == []
    bad = evaluation.ScoreJob("b", np.zeros((6, 96, 96, 3), np.float32), torch.zeros((80, 40)))
    with pytest.raises(ValueError, match="job 'b'"):
        evaluation.lse_many(net, [bad])
    with pytest.raises(ValueError, match="job 'c'"):
        evaluation.lse_many(net, [evaluation.ScoreJob("c", np.zeros((6, 96, 96, 3), np.uint8), torch.zeros((40, 80)))])
    with pytest.raises(ValueError):
        evaluation.lse_many(net, [], batch_size=0)
    with pytest.raises(ValueError):
        evaluation.lse_many(net, [], vshift=128)


def test_parser_has_the_reference_flags_and_defaults():
    """calculate_scores_LRS.py:14-21; --checkpoint_path in place of --initial_model"""
    from wav2lip_amd import calculate_scores as cs
    a = cs.parser.parse_args(["--data_root", "d", "--checkpoint_path", "c.pth"])
    assert (a.batch_size, a.vshift, a.data_root, a.tmp_dir, a.reference) == (20, 15, "d", "data/work/pytmp", "demo")
    assert isinstance(cs.parser.parse_args(["--data_root", "d", "--checkpoint_path", "c", "--vshift", "7"]).vshift, int)
    for missing in (["--checkpoint_path", "c"], ["--data_root", "d"]):
        with pytest.raises(SystemExit):
            cs.parser.parse_args(missing)
    a = cs.cli_parser.parse_args(["--data_root", "d", "--checkpoint_path", "c", "--box", "1", "90", "2", "80", "--fps", "30"])
    assert a.box == [1, 90, 2, 80] and a.fps == 30. and a.face_det_precision == "fp32"
    a = cs.cli_parser.parse_args(["--data_root", "d", "--checkpoint_path", "c"])
    assert a.box is None and a.fps == 25.
