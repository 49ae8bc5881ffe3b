"""LSE-D / LSE-C style lip-sync scoring (BASELINE.json's parity metric) on the HIP path.

The published numbers come from evaluation/scores_LSE/, which wraps the un-vendored `joonson/syncnet_python` model and
weights (`SyncNetModel.S`, data/syncnet_v2.model): not computable offline.  The scoring ARITHMETIC is in the
reference though (SyncNetInstance_calc_scores.py:19-31,95-150), and it only needs two embedding streams.  This module runs
that arithmetic on the embeddings of the in-tree expert `SyncNet_color` (the network the generator is trained against):

    per video frame v: face window = frames v..v+4, lower halves, stacked on channels (wav2lip_train.py:192-195 layout)
                       mel window  = 16 columns from int(80 * v / fps)          (wav2lip_train.py:80)
    dists[i][j] = || face_emb[i] - pad(audio_emb)[i+j] + 1e-6 ||, j over 2*vshift+1 offsets     (calc_pdist :19-31)
    mdist = mean_i dists;  LSE-D = min_j mdist;  LSE-C = median(mdist) - min;  offset = vshift - argmin   (:131-137)

With identical weights on both sides, equal scores for the engine's frames and the CPU path's frames is the stand-in for
"LSE-D / LSE-C parity"; the absolute values are not comparable to the paper's (different scorer network).

`lse_like` scores one clip per call.  `lse_many` scores a whole filelist (evaluation/scores_LSE/calculate_scores_LRS.py:28-50): the
windows of successive clips are rows of SyncNet batches of one size, and a group of clips is scored in one launch;
the group's tables and host faces go up in one staging buffer (staging.py).
"""
import collections

import numpy as np
import torch

from ._lib import LSE_SEGMENT, SYNC_ROW, check, current_stream, load, ptr
from .inference import _precision_kw
from .staging import Staging

syncnet_T = 5
mel_step = 16
img_size = 96

GROUP_BATCHES = 16   # lse_many closes a group of clips once it holds this many full batches of windows

ScoreJob = collections.namedtuple("ScoreJob", "key faces mel first", defaults=(0,))
ScoreJob.__doc__ = """one clip to score: `faces` uint8 [T,96,96,3] face crops (a device tensor or a host array), `mel` the device fp32
[80,Tm] spectrogram (audio.melspectrogram_device); `first` (default 0) the frame of the video the mel belongs to at which the
crops start - a face span of a longer video (calculate_scores_real_videos.py) reads the mel columns of its own frames"""


def sync_windows(frames_u8, mel, fps=25., first=0):
    """frames_u8: torch uint8 [T,96,96,3] generated crops (device); mel: torch float32 [80,Tm] (device).
    Returns (faces [n,15,48,96] float32 in [0,1], mels [n,1,80,16]) for every frame v with a full 5-frame and 16-column
    window.  `first`: the crops start at this frame of the mel's video, so window v reads the columns of frame first + v."""
    T = frames_u8.shape[0]
    H = frames_u8.shape[1]
    x = frames_u8[:, H // 2:].permute(0, 3, 1, 2).float() / 255.           # [T,3,48,96]
    faces, mels = [], []
    for v in range(0, T - syncnet_T + 1):
        s = int(80. * ((first + v) / float(fps)))
        if s + mel_step > mel.shape[1]:
            break
        faces.append(x[v:v + syncnet_T].reshape(3 * syncnet_T, x.shape[2], x.shape[3]))
        mels.append(mel[:, s:s + mel_step].unsqueeze(0))
    if not faces:
        raise ValueError("clip too short for one 5-frame / 16-column window")
    return torch.stack(faces).contiguous(), torch.stack(mels).contiguous()


def lse_from_embeddings(face_emb, audio_emb, vshift=15):
    """SyncNetInstance_calc_scores.py:129-137 on two [n,C] embedding streams -> (offset, LSE-C, LSE-D, mdist [2*vshift+1])"""
    f1 = face_emb.contiguous().float()
    f2 = audio_emb.contiguous().float()
    n, C = f1.shape
    win = 2 * vshift + 1
    d = torch.empty((n, win), device=f1.device, dtype=torch.float32)
    check(load().w2l_shifted_pdist(current_stream(), n, C, vshift, ptr(f1), ptr(f2), ptr(d)), "shifted_pdist")
    mdist = d.mean(dim=0)
    minval, minidx = torch.min(mdist, 0)
    conf = torch.median(mdist) - minval
    return int(vshift - int(minidx)), float(conf), float(minval), mdist


@torch.no_grad()
def lse_like(syncnet, frames_u8, mel, fps=25., vshift=15, batch_size=64, precision="f32", first=0):
    """scores of a generated clip under the in-tree SyncNet_color (eval mode): dict(offset, lse_c, lse_d, n).  `precision`: SyncNet
    arithmetic, "f32" (default) or "bf16" (the opt-in bf16-storage plan; embeddings and scores stay fp32).  `first`: the frame of
    the mel's video at which the crops start (`sync_windows`)"""
    kw = _precision_kw(precision)
    was_training = syncnet.training
    syncnet.eval()
    try:
        faces, mels = sync_windows(frames_u8, mel, fps, first)
        a_all, v_all = [], []
        for lo in range(0, faces.shape[0], batch_size):
            a, v = syncnet(mels[lo:lo + batch_size], faces[lo:lo + batch_size], **kw)
            a_all.append(a)
            v_all.append(v)
        offset, conf, minval, mdist = lse_from_embeddings(torch.cat(v_all), torch.cat(a_all), vshift)
    finally:
        syncnet.train(was_training)
    return dict(offset=offset, lse_c=conf, lse_d=minval, n=int(faces.shape[0]), mdist=mdist.cpu().numpy())


# ---------------------------------------------------------------- many clips, shared SyncNet batches
def sync_rows(T, Tm, fps=25., first=0):
    """the (first frame v, first mel column) of every window `sync_windows` makes of T frames and Tm mel columns: the same
    expression and the same stop rule"""
    rows = []
    for v in range(0, T - syncnet_T + 1):
        s = int(80. * ((first + v) / float(fps)))
        if s + mel_step > Tm:
            break
        rows.append((v, s))
    return rows


def _score_segments(n_seg, segs, vshift, face_emb, audio_emb, out):
    """w2l_lse_score_segments into `out`, fp32 [n_seg * (4 + win)]: the [n_seg][4] scores, then the [n_seg][win] mean distances"""
    check(load().w2l_lse_score_segments(current_stream(), n_seg, ptr(segs), face_emb.shape[1], vshift, ptr(face_emb),
                                        ptr(audio_emb), out.data_ptr() + 16 * n_seg, ptr(out)), "lse_score_segments")


def _score_group(syncnet, clips, vshift, batch_size, precision="f32"):
    """One group on the device.  clips: [(faces, mel, rows)], every `rows` (sync_rows) non-empty.  The windows of the group are
    the rows of one embedding arena pair, clip after clip; batches of exactly `batch_size` rows walk the arena, the last one padded
    with copies of its last row whose embeddings fall into the scratch rows behind the arena.  Returns numpy [clips, 4 + win]:
    (lse_d, lse_c, offset, n) and the mean distances of every clip."""
    dev = clips[0][1].device
    win = 2 * vshift + 1
    W = sum(len(rows) for _, _, rows in clips)
    padded = (W + batch_size - 1) // batch_size * batch_size
    # ---- one staging buffer: [window table, `padded` rows][segment table][host faces of the group]
    st = Staging(dev)
    window_rows, segments = st.table(SYNC_ROW, padded), st.table(LSE_SEGMENT, len(clips))
    src = [st.place(faces) for faces, _, _ in clips]
    st.allocate()
    table, segs = st.view(window_rows), st.view(segments)
    table["pad"] = 0
    frame_bytes = img_size * img_size * 3
    r = 0
    for c, (_, mel, rows) in enumerate(clips):
        vs = np.asarray(rows, dtype=np.int64)
        t = table[r:r + len(rows)]
        t["frames"] = st.address(src[c]) + vs[:, 0] * frame_bytes
        t["mel"], t["T"], t["start"] = mel.data_ptr(), mel.shape[1], vs[:, 1]
        segs[c] = (r, len(rows))
        r += len(rows)
    table[W:] = table[W - 1]
    st.upload()
    audio_emb = torch.empty((padded, 512), dtype=torch.float32, device=dev)     # rows [W, padded): the scratch tail
    face_emb = torch.empty((padded, 512), dtype=torch.float32, device=dev)
    rows_dev = st.tensor(window_rows)
    for lo in range(0, padded, batch_size):
        syncnet.embed_rows(rows_dev[lo * SYNC_ROW.itemsize:(lo + batch_size) * SYNC_ROW.itemsize], batch_size, audio_emb, face_emb, lo,
                           **_precision_kw(precision))
    out = torch.empty(len(clips) * (4 + win), dtype=torch.float32, device=dev)
    _score_segments(len(clips), st.tensor(segments), vshift, face_emb, audio_emb, out)
    res = out.cpu().numpy()                      # the group's one copy back; it also ends the stream's use of the staging buffers
    return np.concatenate([res[:4 * len(clips)].reshape(len(clips), 4), res[4 * len(clips):].reshape(len(clips), win)], axis=1)


def _checked_job(job):
    """(faces, mel) of a ScoreJob: faces a contiguous uint8 [T,96,96,3] device tensor or host array; a ValueError names the job"""
    faces, mel = job.faces, job.mel
    try:
        if not isinstance(mel, torch.Tensor) or mel.dtype != torch.float32 or mel.dim() != 2 or mel.shape[0] != 80:
            raise ValueError("mel must be a float32 [80,Tm] device tensor")
        if isinstance(faces, torch.Tensor):
            if faces.device != mel.device:
                raise ValueError("faces are on %s, mel on %s" % (faces.device, mel.device))
            faces = faces.contiguous()
        else:
            faces = np.ascontiguousarray(faces)
        if faces.dtype not in (torch.uint8, np.uint8) or faces.ndim != 4 or tuple(faces.shape[1:]) != (img_size, img_size, 3):
            raise ValueError("faces must be uint8 [T,%d,%d,3], got %s %s" % (img_size, img_size, faces.dtype, tuple(faces.shape)))
    except ValueError as e:
        raise ValueError("job %r: %s" % (job.key, e)) from None
    return faces, mel.contiguous()


def _checked_first(job):
    """the `first` of a ScoreJob: a non-negative int; a ValueError names the job"""
    first = job.first
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or first < 0:
        raise ValueError("job %r: first must be a non-negative integer, got %r" % (job.key, first))
    return int(first)


@torch.no_grad()
def lse_many(syncnet, jobs, fps=25., vshift=15, batch_size=128, sink=None, precision="f32"):
    """`lse_like` for every `ScoreJob` of the iterable `jobs` (consumed lazily), the windows of successive clips packed into
    SyncNet batches of exactly `batch_size` (evaluation/scores_LSE/calculate_scores_LRS.py:41-47 scores one video per call).

    Jobs are taken until a group holds at least GROUP_BATCHES * batch_size windows or the iterator ends; the group's windows are
    embedded, w2l_lse_score_segments scores all its clips in one launch, one copy brings the scores back, and the group is
    released: the memory alive is one group plus the job being read.  Results arrive in job order as
    dict(key, offset, lse_c, lse_d, n, mdist) - at `sink(result)`, or in the returned list.  A clip without one full window
    gives n = 0 and None for the rest, and takes part in no launch.  A job's `first` places its windows at the mel columns of the
    frames first, first + 1, ... of its video.  The model runs in eval mode and is put back afterwards.
    `precision`: SyncNet arithmetic, "f32" (default) or "bf16" (`SyncNet_color.embed_rows(..., precision="bf16")`)."""
    _precision_kw(precision)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if not 0 <= vshift <= 127:
        raise ValueError("vshift must be in 0..127")
    collected = None
    if sink is None:
        collected = []
        sink = collected.append
    group, windows = [], 0          # (key, faces, mel, rows) of the jobs read since the last group ran

    def flush():
        nonlocal group, windows
        clips = [(faces, mel, rows) for _, faces, mel, rows in group if rows]
        scored = iter(_score_group(syncnet, clips, vshift, batch_size, precision)) if clips else None
        keys = [(key, bool(rows)) for key, _, _, rows in group]
        group, windows = [], 0      # released before the results go out
        del clips
        for key, has_rows in keys:
            if not has_rows:
                sink(dict(key=key, offset=None, lse_c=None, lse_d=None, n=0, mdist=None))
                continue
            row = next(scored)
            sink(dict(key=key, offset=int(row[2]), lse_c=float(row[1]), lse_d=float(row[0]), n=int(row[3]), mdist=row[4:].copy()))

    was_training = syncnet.training
    syncnet.eval()
    try:
        for job in jobs:
            faces, mel = _checked_job(job)
            rows = sync_rows(faces.shape[0], mel.shape[1], fps, _checked_first(job))
            group.append((job.key, faces if rows else None, mel if rows else None, rows))
            del job, faces, mel
            windows += len(rows)
            if windows >= GROUP_BATCHES * batch_size:
                flush()
        if group:
            flush()
    finally:
        syncnet.train(was_training)
    return collected
