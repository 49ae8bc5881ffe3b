"""Generates tests/golden/golden_real_videos_v1.npz from the EXECUTED reference: `get_smoothened_boxes`, `rescale_frames`,
`face_detect`, `datagen`, `increase_frames` and `main` of the reference's evaluation/real_videos_inference.py, their source taken
out of the file with `ast` (the module parses sys.argv and loads a detector and a model at import) and run as written on CPU
fp32, in `tts` mode.  Runs only in the build container.

    python tests/golden/make_golden_real_videos.py

The namespace is the one tests/golden/make_golden_filelist.py builds: the reference's own `audio` (librosa stubs, the numpy-1.17
promotion shim), its `face_detection.FaceAlignment` with the seeded S3FD weights, its `models.Wav2Lip` with the seeded generator
weights, `args` parsed by the reference's own parser statements, and stubs that hold no arithmetic of the path: `cv2.VideoCapture`
serves the seeded clips of wav2lip_amd.synthetic.real_video_clips and their frame rates, `cv2.VideoWriter` collects frames,
`subprocess.call` records which audio source the "ffmpeg" extraction named and which result file the mux wrote, `tqdm` is the
identity, `dlib` and the other unused imports are never executed.  `cv2.resize` is oracle.resize_ref, the OpenCV restatement.

Flags (synthetic.REAL_FLAGS): small resolutions, so that both whole-frame resizes fire on small frames; asserted below.

Recorded: the frozen argparse surface; per line written or skipped, the frame size as read, after the `max_frame_res` cap and
after `rescale_frames`, the chosen factor, the index list of `increase_frames`, the smoothed boxes; the chunk starts the loop of
:248-255 gives at 25, 30 and 23.976 fps (that `while` statement, executed on a recording spectrogram); tables of `increase_frames`
index lists and `rescale_frames` factors over grids of small arguments (the functions as written, a fixed-rect detector for the
second); the output frames of the first and last row of every written clip and of the rows on both sides of every packed-batch
boundary at batch 16 as box regions (the script asserts that everything outside the box equals the rescaled input frame), and a
per-frame mean of every output frame.

Asserted here, so that fp32 rounding alone cannot flip a decision: on every frame the detector saw in a written clip (frame 0 at
the capped size, every frame at the final size) every float box coordinate inside the frame is at least 0.01 from an integer and
the best detector score is at least 0.04 from the 0.5 threshold; the skipped clip's first frame scores at least 0.04 below it.
"""
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
REF = "/root/reference"
REF_FILE = os.path.join(REF, "evaluation", "real_videos_inference.py")

from oracle import resize_ref  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402

BATCH = 16
FPS_TABLE = (25., 30., 23.976)
MEL_TABLE = (15, 16, 17, 19, 20, 45, 80, 133, 241, 500)
INCREASE_GRID = [(n, l) for n in range(1, 13) for l in sorted({n, n + 1, n + 2, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n + 1, 5 * n + 3, 29})
                 if l >= n]
FACTOR_GRID = [(face, h, w, face_res, min_res) for face in (20, 47, 50, 100, 180, 200, 359, 360, 400, 700, 1000, 3000)
               for h, w in ((720, 1280), (1080, 1920), (480, 640), (144, 192)) for face_res in (180, 24, 96) for min_res in (480, 60, 1)]


def reference_source():
    src = open(REF_FILE).read()
    body = ast.parse(src).body
    fns = {n.name: ast.get_source_segment(src, n) for n in body if isinstance(n, ast.FunctionDef)}
    stmts = [ast.get_source_segment(src, n) for n in body
             if (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "parser")
             or (isinstance(n, ast.Expr) and isinstance(n.value, ast.Call) and getattr(n.value.func, "attr", "") == "add_argument")]
    # the chunking loop of main(): the `while` statement that appends to mel_chunks (:250-255)
    main = [n for n in body if isinstance(n, ast.FunctionDef) and n.name == "main"][0]
    loops = [n for n in ast.walk(main) if isinstance(n, ast.While) and "mel_chunks.append" in ast.get_source_segment(src, n)]
    assert len(loops) == 1
    lines = src.splitlines()[loops[0].lineno - 1:loops[0].end_lineno]
    indent = len(lines[0]) - len(lines[0].lstrip())
    return fns, "\n".join(stmts), "\n".join(l[indent:] for l in lines)


class RecordingMel:
    """stands for `mel` in the chunking loop: len(mel[0]) columns, mel[:, a:b] records a"""

    def __init__(self, n):
        self.n, self.starts = n, []

    def __getitem__(self, key):
        if isinstance(key, tuple):
            self.starts.append(int(key[1].start))
            assert key[1].stop - key[1].start == 16
            return None
        assert key == 0
        return range(self.n)


def main():
    import make_golden_datapath as mgd
    torch.set_num_threads(8)
    torch.manual_seed(0)
    mgd.install_stubs({})
    del sys.modules["face_detection"]
    sys.path.insert(0, REF)
    import audio as ref_audio
    import face_detection
    import models as ref_models
    from face_detection.detection.sfd import sfd_detector
    from face_detection.detection.sfd.detect import batch_detect
    assert ref_audio.__file__.startswith(REF) and face_detection.__file__.startswith(REF) and ref_models.__file__.startswith(REF)

    class _Numpy117(types.ModuleType):                      # numpy==1.17.1 promotion at audio.py:104-105 (make_golden_datapath.py)
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def exp(x):
            r = np.exp(x)
            return float(r) if np.ndim(r) == 0 else r
    ref_audio.np = _Numpy117("numpy")

    clips = synth.real_video_clips()
    state = {"audio_src": None, "frames": None, "results": {}, "fps": None}

    class VideoCapture:
        def __init__(self, vfile):
            name = os.path.basename(vfile)
            self.frames = [f.copy() for f in clips[name][0]]
            self.fps = clips[name][1]

        def get(self, prop):
            assert prop == "CAP_PROP_FPS"
            return self.fps

        def read(self):
            return (True, self.frames.pop(0)) if self.frames else (False, None)

        def release(self):
            pass

    class VideoWriter:
        def __init__(self, path, fourcc, fps, size):
            state["frames"] = []
            state["size"] = size
            state["fps"] = fps

        def write(self, f):
            state["frames"].append(f.copy())

        def release(self):
            pass

    def call(command, shell=False):
        parts = command.split()
        if parts[-1] == '../temp/temp.wav':                 # the extraction: remember whose audio temp.wav now holds
            state["audio_src"] = os.path.basename(parts[parts.index('-i') + 1])
        else:                                               # the mux: the collected frames become result <idx>
            idx = int(os.path.basename(parts[-1]).split('.')[0])
            state["results"][idx] = (np.stack(state["frames"]), state["size"], state["fps"])
        return 0

    def load(path, sr=22050):
        assert sr == 16000 and path == '../temp/temp.wav'
        pcm = clips[state["audio_src"]][2]
        return pcm[:, 0].astype(np.float32) / np.float32(32768.0), sr
    sys.modules["librosa"].core.load = load

    resizes = []
    cv2 = types.ModuleType("cv2")
    cv2.VideoCapture, cv2.VideoWriter = VideoCapture, VideoWriter
    cv2.VideoWriter_fourcc = lambda *a: 0
    cv2.CAP_PROP_FPS = "CAP_PROP_FPS"

    def resize(img, dsize):
        resizes.append((tuple(img.shape[:2]), tuple(int(v) for v in dsize)))
        return resize_ref.resize_linear_u8(img, dsize)
    cv2.resize = resize

    sd_det = synth.s3fd_state_dict()
    sfd_detector.load_url = lambda url: sd_det
    detector = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device="cpu")
    net = ref_models.Wav2Lip()
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=0)
    net.load_state_dict(sd)
    net = net.eval()

    fns, parser_src, chunk_loop = reference_source()
    import argparse
    pns = {"argparse": argparse}
    exec(parser_src, pns)
    n_lines = len(synth.REAL_LINES)
    with tempfile.TemporaryDirectory() as tmp:
        filelist = os.path.join(tmp, "list.txt")
        with open(filelist, "w") as fh:
            fh.write("".join("%s %s\n" % l for l in synth.REAL_LINES))
        # the reference declares no type for the three resolutions: given on the command line they arrive as strings.  The surface
        # is recorded as parsed; the values are then set as the ints its defaults are
        args = pns["parser"].parse_args(["--mode", "tts", "--filelist", filelist, "--results_dir", os.path.join(tmp, "results"),
                                         "--data_root", "data", "--checkpoint_path", "none", "--wav2lip_batch_size", str(BATCH)]
                                        + synth.REAL_FLAGS)
        assert isinstance(args.max_frame_res, str)
        for name in ("face_res", "min_frame_res", "max_frame_res"):
            setattr(args, name, int(getattr(args, name)))
        args.img_size = 96
        subprocess = types.ModuleType("subprocess")
        subprocess.call = call
        ns = {"args": args, "np": np, "cv2": cv2, "os": os, "subprocess": subprocess, "tqdm": lambda x: x, "audio": ref_audio,
              "detector": detector, "model": net, "torch": torch, "device": "cpu", "mel_step_size": 16, "listdir": os.listdir}
        for name in ("get_smoothened_boxes", "rescale_frames", "face_detect", "datagen", "increase_frames", "main"):
            exec(fns[name], ns)
        real = {k: ns[k] for k in ("face_detect", "rescale_frames", "increase_frames")}
        order, seen, dups = [], [], []

        def recording_face_detect(images):
            given = [im.copy() for im in images]
            seen.append(given)                                                   # every call, also one that raises
            res, out_images = real["face_detect"](images)
            order.append((given, [im.copy() for im in out_images], [tuple(int(v) for v in r[1]) for r in res]))
            return res, out_images

        def recording_increase_frames(frames, l):
            dups.append((len(seen), real["increase_frames"](list(range(len(frames))), l)))
            return real["increase_frames"](frames, l)
        ns["face_detect"], ns["increase_frames"] = recording_face_detect, recording_increase_frames
        ns["main"]()

        # ---- the tables: the functions as written, over grids of small arguments
        inc = [real["increase_frames"](list(range(n)), l) for n, l in INCREASE_GRID]
        factors = []
        for face, h, w, face_res, min_res in FACTOR_GRID:
            targs = types.SimpleNamespace(face_res=face_res, min_frame_res=min_res)
            tdet = types.SimpleNamespace(get_detections_for_batch=lambda b, face=face: [(3, 5, 3 + face // 2, 5 + face)])
            got = []
            tcv2 = types.SimpleNamespace(resize=lambda im, dsize: got.append(dsize) or im)
            tns = {"args": targs, "np": np, "cv2": tcv2, "detector": tdet}
            exec(fns["rescale_frames"], tns)
            tns["rescale_frames"]([np.zeros((h, w, 3), np.uint8)])
            if not got:
                factors.append(1)
            else:
                f = [f for f in range(2, 16) if (w // f, h // f) == tuple(got[0])]
                assert len(f) == 1, (face, h, w, got)
                factors.append(f[0])
        chunk_starts = {}
        for fps in FPS_TABLE:
            for n_mel in MEL_TABLE:
                mel = RecordingMel(n_mel)
                exec(chunk_loop, {"mel": mel, "mel_chunks": [], "i": 0, "mel_idx_multiplier": 80. / fps, "mel_step_size": 16,
                                  "len": len, "int": int})
                chunk_starts[(fps, n_mel)] = mel.starts

    written = sorted(state["results"])
    assert written == [0, 1, 2, 4, 5], written
    assert len(order) == len(written) and len(seen) == n_lines
    out = {"written": np.asarray([int(i in state["results"]) for i in range(n_lines)], np.int64), "batch_size": np.int64(BATCH),
           "cli": np.array(json.dumps(mgd.parser_surface(pns["parser"]))), "flags": np.array(json.dumps(synth.REAL_FLAGS)),
           "n_frames": np.asarray([len(state["results"][i][0]) if i in state["results"] else 0 for i in range(n_lines)], np.int64),
           "fps": np.asarray([state["results"][i][2] if i in state["results"] else 0. for i in range(n_lines)], np.float64),
           "increase_grid": np.asarray(INCREASE_GRID, np.int64), "increase_index": np.concatenate([np.asarray(x, np.int64) for x in inc]),
           "factor_grid": np.asarray(FACTOR_GRID, np.int64), "factor_table": np.asarray(factors, np.int64),
           "chunk_fps": np.asarray(FPS_TABLE), "chunk_n_mel": np.asarray(MEL_TABLE, np.int64)}
    assert all(len(x) == l for x, (_, l) in zip(inc, INCREASE_GRID)) and len(set(factors)) >= 5, sorted(set(factors))
    for k, fps in enumerate(FPS_TABLE):
        for n_mel in MEL_TABLE:
            out["chunks_%d_%d" % (k, n_mel)] = np.asarray(chunk_starts[(fps, n_mel)], np.int64)
    assert out["n_frames"].tolist() == [10, 14, 11, 0, 10, 10], out["n_frames"].tolist()

    # ---- sizes, factors, index lists per line (lines in `seen` order = line order: face_detect is called once per line)
    size_read = np.zeros((n_lines, 2), np.int64)
    size_capped = np.zeros((n_lines, 2), np.int64)
    size_final = np.zeros((n_lines, 2), np.int64)
    factor = np.zeros(n_lines, np.int64)
    dup_of = {k: idx for k, idx in dups}
    for i, (video, _) in enumerate(synth.REAL_LINES):
        size_read[i] = clips[video][0].shape[1:3]
        size_capped[i] = seen[i][0].shape[:2]
        index = dup_of.get(i, list(range(len(seen[i]))))
        out["index_%d" % i] = np.asarray(index, np.int64)
        assert len(index) == len(seen[i])
        for k, j in enumerate(index):                                           # the frames given are the capped frames [index]
            if tuple(size_read[i]) == tuple(size_capped[i]):
                assert np.array_equal(seen[i][k], clips[video][0][j])
    for (given, images, boxes), i in zip(order, written):
        size_final[i] = images[0].shape[:2]
        h, w = given[0].shape[:2]
        f = [f for f in range(1, 16) if (h // f, w // f) == tuple(size_final[i])]
        assert len(f) == 1, (i, h, w, size_final[i])
        factor[i] = f[0]
    out.update(size_read=size_read, size_capped=size_capped, size_final=size_final, factor=factor)
    print("read", size_read.tolist(), "capped", size_capped.tolist(), "final", size_final.tolist(), "factor", factor.tolist())
    # both resizes fired, on one clip at least; one clip took neither; two shapes; both kinds of shortfall
    assert any((size_read[i] != size_capped[i]).any() and factor[i] > 1 for i in written)
    assert any((size_read[i] == size_final[i]).all() for i in written)
    assert len({tuple(size_final[i]) for i in written}) >= 2
    assert sorted(dup_of) == [2, 4] and len(clips["r2"][0]) * 2 > 11 and len(clips["r3"][0]) * 2 < 10
    assert any(src == (180, 240) for src, _ in resizes) and any(src == (144, 192) and dst == (96, 72) for src, dst in resizes)

    # ---- margins on every frame the detector saw in a written clip, and the skipped clip's decision
    def margins(frames):
        fr = np.asarray(frames)
        dense = batch_detect(detector.face_detector.face_detector, fr[..., ::-1].copy(), device="cpu")
        lists = detector.face_detector.detect_from_batch(fr[..., ::-1].copy())
        for k, d in enumerate(lists):
            best = float(dense[:, k, 4].max())
            assert abs(best - 0.5) >= 0.04, (k, best)
            if len(d) == 0:
                continue
            b = np.asarray(d[0][:4], np.float64)
            H, W = fr.shape[1:3]
            inside = np.array([b[0] < W, b[1] < H, b[2] < W, b[3] < H]) & (b > 0)
            frac = np.abs(b - np.round(b))[inside]
            assert frac.size == 0 or frac.min() >= 0.01, (k, b)
        return [len(d) > 0 for d in lists]
    for (given, images, _), idx in zip(order, written):
        assert all(margins(given[:1])) and all(margins(images)), idx
    assert margins(seen[3][:1]) == [False]

    # ---- frames: box regions of the first / last row of every clip and of both sides of every packed-batch boundary
    row0 = 0
    for (given, images, boxes), idx in zip(order, written):
        frames, size, _ = state["results"][idx]
        n = len(frames)
        assert size == (images[0].shape[1], images[0].shape[0]) and len(boxes) == n == len(images)
        out["boxes_%d" % idx] = np.asarray(boxes, np.int64)                         # (y1, y2, x1, x2), smoothed
        out["mean_%d" % idx] = frames.reshape(n, -1).astype(np.float64).mean(axis=1)
        keep = {0, n - 1}
        for r in range(n):
            g = row0 + r
            if g % BATCH == 0 or g % BATCH == BATCH - 1:
                keep.add(r)
        keep = sorted(keep)
        out["rows_%d" % idx] = np.asarray(keep, np.int64)
        for r in keep:
            y1, y2, x1, x2 = boxes[r]
            outside = frames[r].copy()
            outside[y1:y2, x1:x2] = images[r][y1:y2, x1:x2]
            assert np.array_equal(outside, images[r])                               # outside the box: the rescaled input frame
            out["face_%d_%d" % (idx, r)] = frames[r][y1:y2, x1:x2].copy()
        row0 += n
    assert row0 == 55

    path = os.path.join(HERE, "golden_real_videos_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %.1f kB" % (path, len(out), os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) <= 593594                                          # the largest golden committed so far
    for idx in written:
        print(idx, out["rows_%d" % idx].tolist(), out["index_%d" % idx].tolist(), out["boxes_%d" % idx][:3].tolist())


if __name__ == "__main__":
    main()
