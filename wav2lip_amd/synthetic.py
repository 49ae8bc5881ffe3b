"""Seeded synthetic weights and inputs for benchmarks, smoke() and the tests (numpy PCG64: stable across torch versions, so
the committed golden outputs stay valid).  There is no network here for datasets or checkpoints: bench.py and
tools/*_bench.py build their workloads from this module.  Pure data generation, no reference arithmetic.

Weights: He-scaled conv kernels, small biases and *randomised* BatchNorm statistics (fresh-init BN is nearly the
identity and would hide BN-fusion bugs).  Inputs follow SURVEY.md section 8(d).
"""
import re
import zlib

import numpy as np
import torch


_CONVT = re.compile(r"face_decoder_blocks\.[1-6]\.0\.conv_block\.0\.weight$")


def _rng(seed, key):
    return np.random.default_rng([seed, zlib.crc32(key.encode())])


def synthetic_state_dict(shapes, seed=0):
    """shapes: {key: shape} in reference state-dict naming -> {key: torch tensor}"""
    sd = {}
    for key, shape in shapes.items():
        r = _rng(seed, key)
        shape = tuple(shape)
        if key.endswith("num_batches_tracked"):
            v = np.array(100, dtype=np.int64)
        elif key.endswith("running_mean"):
            v = r.normal(0.0, 0.1, shape)
        elif key.endswith("running_var"):
            v = r.uniform(0.6, 1.4, shape)
        elif ".conv_block.1." in key and key.endswith("weight"):   # BN gamma
            v = r.uniform(0.7, 1.1, shape)
        elif ".conv_block.1." in key and key.endswith("bias"):     # BN beta
            v = r.normal(0.0, 0.1, shape)
        elif key.endswith("weight"):                                # conv / convT kernels
            if _CONVT.match(key):                                   # [cin, cout, k, k]; ~k*k/s^2 taps per output
                fan_in = shape[0] * (1.0 if shape[0] == 1024 and "blocks.1." in key else 2.25)
            else:
                fan_in = int(np.prod(shape[1:]))
            v = r.normal(0.0, np.sqrt(1.0 / max(fan_in, 1)), shape)
        else:                                                       # conv bias
            v = r.normal(0.0, 0.05, shape)
        sd[key] = torch.from_numpy(np.asarray(v, dtype=np.int64 if v.dtype == np.int64 else np.float32).copy())
    return sd


def face_crops_u8(n, seed=0, size=96):
    """uint8 BGR crops [n, size, size, 3]"""
    return _rng(seed, "faces").integers(0, 256, (n, size, size, 3), dtype=np.uint8)


def mel_windows(n, seed=0):
    """[n, 80, 16] float32 in the normalised mel range U(-4, 4)"""
    return _rng(seed, "mel").uniform(-4.0, 4.0, (n, 80, 16)).astype(np.float32)


def sine_wav(seconds=3.0, freq=440.0, sr=16000, amp=0.5):
    """config-1 audio: sine written as PCM16 and read back the way librosa/soundfile does (int16 / 32768)"""
    t = np.arange(int(seconds * sr)) / sr
    pcm = np.round(amp * np.sin(2 * np.pi * freq * t) * 32767.0).astype(np.int16)
    return (pcm.astype(np.float32) / 32768.0).astype(np.float32)


def noise_wav(nsamples, seed=0):
    return _rng(seed, "noise").uniform(-1.0, 1.0, nsamples).astype(np.float32)


def sync_faces(n, seed=0):
    """SyncNet face input [n, 15, 48, 96] U(0,1)"""
    return _rng(seed, "syncfaces").uniform(0.0, 1.0, (n, 15, 48, 96)).astype(np.float32)


def disc_frames(n, t, seed=0):
    """[n, 3, t, 96, 96] U(0,1)"""
    return _rng(seed, "discframes").uniform(0.0, 1.0, (n, 3, t, 96, 96)).astype(np.float32)


# ---------------------------------------------------------------- S3FD (no s3fd.pth offline)
_S3FD_CONVS = [("conv1_1", 3, 64, 3), ("conv1_2", 64, 64, 3), ("conv2_1", 64, 128, 3), ("conv2_2", 128, 128, 3),
               ("conv3_1", 128, 256, 3), ("conv3_2", 256, 256, 3), ("conv3_3", 256, 256, 3), ("conv4_1", 256, 512, 3),
               ("conv4_2", 512, 512, 3), ("conv4_3", 512, 512, 3), ("conv5_1", 512, 512, 3), ("conv5_2", 512, 512, 3),
               ("conv5_3", 512, 512, 3), ("fc6", 512, 1024, 3), ("fc7", 1024, 1024, 1), ("conv6_1", 1024, 256, 1),
               ("conv6_2", 256, 512, 3), ("conv7_1", 512, 128, 1), ("conv7_2", 128, 256, 3)]
_S3FD_NORMS = [("conv3_3_norm", 256, 10.), ("conv4_3_norm", 512, 8.), ("conv5_3_norm", 512, 5.)]
_S3FD_HEADS = [("conv3_3_norm", 256, 4), ("conv4_3_norm", 512, 2), ("conv5_3_norm", 512, 2), ("fc7", 1024, 2), ("conv6_2", 512, 2),
               ("conv7_2", 256, 2)]


def s3fd_state_dict(seed=0):
    """He-scaled VGG trunk (first layer divided by 128: pixel values are O(128)), small heads with a background-leaning conf
    bias: a detector that fires on a few positions only, in the reference's state-dict naming"""
    r = np.random.default_rng(seed)
    sd = {}
    for name, cin, cout, k in _S3FD_CONVS:
        sd[name + ".weight"] = torch.from_numpy(r.normal(0, np.sqrt(2.0 / (cin * k * k)), (cout, cin, k, k)).astype(np.float32))
        sd[name + ".bias"] = torch.from_numpy(r.normal(0, 0.05, cout).astype(np.float32))
    sd["conv1_1.weight"] = sd["conv1_1.weight"] / 128.0
    for name, c, scale in _S3FD_NORMS:
        sd[name + ".weight"] = torch.from_numpy((scale * r.uniform(0.8, 1.2, c)).astype(np.float32))
    for src, cin, ncls in _S3FD_HEADS:
        sd[src + "_mbox_conf.weight"] = torch.from_numpy(r.normal(0, 0.02, (ncls, cin, 3, 3)).astype(np.float32))
        b = r.normal(0, 0.05, ncls).astype(np.float32)
        b[-1] -= 1.0
        sd[src + "_mbox_conf.bias"] = torch.from_numpy(b)
        sd[src + "_mbox_loc.weight"] = torch.from_numpy(r.normal(0, 0.02, (4, cin, 3, 3)).astype(np.float32))
        sd[src + "_mbox_loc.bias"] = torch.from_numpy(r.normal(0, 0.05, 4).astype(np.float32))
    return sd


def s3fd_frames(seed=1, B=2, H=96, W=128):
    """uint8 BGR frames with one saturated block each (drives a few detector positions above the 0.5 threshold)"""
    r = np.random.default_rng(seed)
    img = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    img[0, 20:60, 30:90] = 255
    if B > 1:
        img[1, 40:80, 10:70] = 0
    return img


def preprocess_frames(n, seed, H=160, W=160):
    """uint8 BGR frames of a synthetic clip for the preprocessing path (LRS2 frames are 160x160): most are noise with one saturated
    block at a seeded place - the seeded S3FD (s3fd_state_dict) finds a "face" there, well above the 0.5 threshold - and about one in
    four is flat grey (120) with faint noise, on which it finds none"""
    r = _rng(seed, "preprocess")
    out = np.empty((n, H, W, 3), np.uint8)
    for k in range(n):
        if r.uniform() < 0.25:
            out[k] = 120 + r.integers(-1, 2, (H, W, 3))
            continue
        out[k] = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
        h, w = r.integers(H // 4, H // 2), r.integers(W // 4, W // 2)
        y, x = r.integers(0, H - h), r.integers(0, W - w)
        out[k, y:y + h, x:x + w] = 255 if r.uniform() < 0.5 else 0
    return out


# (directory, clip name, frames, audio channels, audio rate): two directories, clip lengths that leave a ragged last batch at
# batch size 4, a stereo track at another rate, and a clip without audio
PREPROCESS_CLIPS = [("spk1", "00001", 11, 1, 16000), ("spk1", "00002", 5, 2, 22050), ("spk2", "00003", 9, 1, 16000),
                    ("spk2", "00004", 3, 0, 0)]


def preprocess_clips(seed=4, fps=25):
    """[(directory, clip name, frames uint8 [T,160,160,3] BGR, audio int16 [n, channels] or None, audio rate)] of PREPROCESS_CLIPS"""
    clips = []
    for i, (d, name, t, ch, sr) in enumerate(PREPROCESS_CLIPS):
        frames = preprocess_frames(t, seed * 100 + i)
        pcm = None
        if ch:
            n = t * sr // fps
            pcm = _rng(seed * 100 + i, "preprocess_audio").integers(-8000, 8000, (n, ch)).astype(np.int16)
        clips.append((d, name, frames, pcm, sr))
    return clips


# ---------------------------------------------------------------- training batches at the BASELINE launch shapes
def train_batch(cfg, B, seed=0, T=5):
    """Seeded inputs of one training step (BASELINE configs[2..4]; the committed goldens of tests/golden/
    make_golden_train_baseline.py, the GPU tests at those shapes and tools/train_bench.py's in-run parity check all call this).
      cfg 3: {"x": [B,15,48,96] U(0,1), "mel": [B,1,80,16] U(-4,4), "y": [B,1] alternating 1, 0}     color_syncnet_train.py:155-165
      cfg 4 / 5: {"x": [B,6,T,96,96] (masked ground truth | wrong window), "indiv_mels": [B,T,1,80,16], "mel": [B,1,80,16],
                  "gt": [B,3,T,96,96]}                                      wav2lip_train.py:220-231, hq_wav2lip_train.py:221-256"""
    if cfg == 3:
        y = np.zeros((B, 1), np.float32)
        y[0::2] = 1.0
        return {"x": sync_faces(B, seed), "mel": mel_windows(B, seed)[:, None], "y": y}
    if cfg not in (4, 5):
        raise ValueError("train_batch: cfg must be 3, 4 or 5")
    r = _rng(seed, "trainbatch")
    gt = r.uniform(0.0, 1.0, (B, 3, T, 96, 96)).astype(np.float32)
    wrong = r.uniform(0.0, 1.0, (B, 3, T, 96, 96)).astype(np.float32)
    masked = gt.copy()
    masked[:, :, :, 48:] = 0.0
    return {"x": np.concatenate([masked, wrong], axis=1),
            "indiv_mels": r.uniform(-4.0, 4.0, (B, T, 1, 80, 16)).astype(np.float32),
            "mel": r.uniform(-4.0, 4.0, (B, 1, 80, 16)).astype(np.float32), "gt": gt}


def sketch_vectors(name, n, k=4):
    """k fixed +-1 vectors of length n for parameter `name`: the inner products of a gradient with them ("sketches") pin its
    DIRECTION in a golden file that cannot hold the tensor (E <d, r>^2 = |d|^2 for a difference d)"""
    r = np.random.default_rng([77, zlib.crc32(name.encode())])
    return r.integers(0, 2, (k, n), dtype=np.int8) * 2 - 1


# ---------------------------------------------------------------- filelist generation (evaluation/gen_videos_from_filelist.py)
FILELIST_SHAPES = [(160, 160), (128, 144)]      # (H, W) of the two frame shapes
FILELIST_POOL = 6                                # distinct frames per shape; a clip cycles through its shape's pool
# (clip name, shape index, frames, mel chunks of its audio, index of a face-less frame or None)
FILELIST_CLIPS = [("c0", 0, 39, 37, None), ("c1", 1, 61, 61, None), ("c2", 1, 3, 9, None), ("c3", 0, 52, 50, None),
                  ("c4", 1, 20, 18, 7), ("c5", 0, 10, 20, None)]
# (audio source, video) per filelist line: 37, skipped (a face-less frame), 61, 9 (another clip's audio), skipped (fewer frames than
# chunks), 50 rows: at batch 32 the packed batches are 32, 32, 32, 32, 29; the second holds rows of two clips, the fourth of three
FILELIST_LINES = [("c0", "c0"), ("c4", "c4"), ("c1", "c1"), ("c2", "c0"), ("c5", "c5"), ("c3", "c3")]


def filelist_frame(seed, H, W):
    """one uint8 BGR noise frame with a saturated block at a seeded place: the seeded S3FD finds a "face" there"""
    r = _rng(seed, "filelist")
    out = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    h, w = r.integers(H // 4, H // 2), r.integers(W // 4, W // 2)
    y, x = r.integers(0, H - h), r.integers(0, W - w)
    out[y:y + h, x:x + w] = 255 if r.uniform() < 0.5 else 0
    return out


def filelist_samples(n_chunks):
    """audio samples whose spectrogram (1 + n // 200 columns) holds exactly `n_chunks` full 16-column windows at 25 fps"""
    return (int((n_chunks - 1) * 3.2) + 16 - 1) * 200 + 50


def filelist_clips(seed=3):
    """{clip name: (frames uint8 [T,H,W,3] BGR, mono PCM16 audio int16 [n,1] at 16 kHz)} of FILELIST_CLIPS"""
    pools = [[filelist_frame(seed * 1000 + 10 * s + k, H, W) for k in range(FILELIST_POOL)] for s, (H, W) in enumerate(FILELIST_SHAPES)]
    clips = {}
    for i, (name, s, t, chunks, faceless) in enumerate(FILELIST_CLIPS):
        frames = np.stack([pools[s][(k + i) % FILELIST_POOL] for k in range(t)])
        if faceless is not None:
            H, W = FILELIST_SHAPES[s]
            frames[faceless] = 120 + _rng(seed * 1000 + i, "filelist_grey").integers(-1, 2, (H, W, 3))
        pcm = _rng(seed * 1000 + i, "filelist_audio").integers(-8000, 8000, (filelist_samples(chunks), 1)).astype(np.int16)
        clips[name] = (frames, pcm)
    return clips


# ---------------------------------------------------------------- real-video generation (evaluation/real_videos_inference.py)
REAL_SHAPES = [(180, 240), (168, 216), (72, 96)]        # (H, W): the first two exceed --max_frame_res 144, the third does not
# seeds of the distinct frames per shape (a clip cycles through its shape's pool), picked so that the seeded S3FD's decisions on
# them - at the size the detector sees them - keep the margins tests/golden/make_golden_real_videos.py asserts
REAL_FRAME_SEEDS = [[5000, 5001, 5002, 5006], [5100, 5101, 5102, 5103], [5200, 5201, 5202, 5203]]
REAL_POOL = 4
# (clip name, shape index, frames, mel chunks of its audio at its fps, fps, first frame face-less?)
REAL_CLIPS = [("r0", 2, 12, 10, 25., False), ("r1", 0, 14, 14, 25., False), ("r2", 1, 9, 11, 25., False), ("r3", 2, 4, 4, 25., False),
              ("r4", 0, 8, 8, 25., True), ("r5", 1, 10, 10, 30., False)]
# (video, audio source) per line, run in `tts` mode with REAL_FLAGS: 10 rows (neither resize), 14 (both resizes), 11 from 9 frames
# (two duplicated), skipped (no face in the first frame), 10 from 4 frames (duplicated twice over), 10 at 30 fps
REAL_LINES = [("r0", "r0"), ("r1", "r1"), ("r2", "r2"), ("r4", "r4"), ("r3", "r0"), ("r5", "r5")]
REAL_FLAGS = ["--max_frame_res", "144", "--min_frame_res", "60", "--face_res", "24", "--face_det_batch_size", "4"]


def real_frame(seed, H, W):
    """one uint8 BGR noise frame with a saturated block about half the frame high at a seeded place (the seeded S3FD's "face")"""
    r = _rng(seed, "real_videos")
    out = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    h, w = r.integers(9 * H // 20, 11 * H // 20), r.integers(9 * H // 20, 11 * H // 20)
    y, x = r.integers(H // 8, H - h - H // 8), r.integers(W // 8, W - w - W // 8)
    out[y:y + h, x:x + w] = 255 if r.uniform() < 0.5 else 0
    return out


def real_samples(n_chunks, fps):
    """audio samples whose spectrogram (1 + n // 200 columns) holds exactly `n_chunks` full 16-column windows at `fps`"""
    return (int((n_chunks - 1) * (80. / fps)) + 16 - 1) * 200 + 50


def real_video_clips(seed=5):
    """{clip name: (frames uint8 [T,H,W,3] BGR, fps, mono PCM16 audio int16 [n,1] at 16 kHz)} of REAL_CLIPS"""
    pools = [[real_frame(k, H, W) for k in REAL_FRAME_SEEDS[s]] for s, (H, W) in enumerate(REAL_SHAPES)]
    clips = {}
    for i, (name, s, t, chunks, fps, faceless) in enumerate(REAL_CLIPS):
        frames = np.stack([pools[s][(k + i) % REAL_POOL] for k in range(t)])
        if faceless:
            H, W = REAL_SHAPES[s]
            frames[0] = 120 + _rng(seed * 1000 + i, "real_videos_grey").integers(-1, 2, (H, W, 3))
        pcm = _rng(seed * 1000 + i, "real_videos_audio").integers(-8000, 8000, (real_samples(chunks, fps), 1)).astype(np.int16)
        clips[name] = (frames, fps, pcm)
    return clips
