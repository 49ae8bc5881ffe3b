"""Scene-cut detection (opt-in): every shot of a clip is boxed and tracked alone, instead of treating the clip as one
continuous take as the reference does (inference.py:59-66 smooths, and the hold and the track of 3v / 3w look back, across a cut).

The rule, with one threshold `thresh` in [1/256, 1) quantised to q = int(thresh * 256) in 1..255 - what w2l_frame_hist_rows and
w2l_scene_cuts (csrc/scene.hip, include/w2l_hip.h) compute on the device, stated here on the host beside each of them:

    signature of a frame    `host_signatures`: the frame is H * W * 3 contiguous bytes, BGR interleaved; byte j belongs to channel
                            j % 3 and bin byte >> 3; sig[c * 32 + b] counts them - 96 words, integers only, no luma, no float
    distance                D(i) = sum_k |sig_i[k] - sig_{i-1}[k]|, in 0 .. 6 * H * W
    cut                     `host_cut_flags`: frame i >= 1 starts a new shot iff D(i) * 256 > q * 6 * H * W; frame 0 never does.
                            One frame back only: causal.
    shots                   `split_shots`: every maximal range [a, b) between cuts is handled as a clip of those frames alone - a fresh
                            track, a hold that does not look back past a, pads, clipping and smoothing per shot

Gradual transitions (fades, dissolves) are not detected.  There is no default threshold: no footage is behind one.  0.3 is a
starting point and a choice, not a measurement; `python -m wav2lip_amd.face_detection.scene VIDEO.avi [--scene_cuts T]` prints the
per-frame distance D / (6 * H * W) of a video (and the cut frames for T) to pick one by.
"""
import collections

import numpy as np

from .._lib import BOX_SEGMENT  # noqa: F401  -- the segment table of w2l_scene_cuts

SIG_WORDS, SIG_BINS = 96, 32

SceneCuts = collections.namedtuple("SceneCuts", "thresh")
SceneCuts.__doc__ = """scene-cut detection: `thresh` in [1/256, 1), the fraction of the largest possible signature distance above which a
frame starts a new shot (quantised to q/256).  There is no default: it is a choice, not a measurement."""


def scene_q8(thresh):
    """`q` of the cut rule for a `thresh`: int(thresh * 256), as `track.iou_q8` quantises"""
    return int(thresh * 256)


def check_scene(value):
    """the `scene_cuts=` of `face_detect` and `detect_many`: None (the reference's one take per clip), a threshold, or a SceneCuts.
    Returns None or a SceneCuts of a float; a ValueError names what is wrong."""
    if value is None:
        return None
    thresh = value.thresh if isinstance(value, SceneCuts) else value
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.integer, np.floating)):
        raise ValueError("scene_cuts must be None, a threshold in [1/256, 1) or a SceneCuts, got %r" % (value,))
    thresh = float(thresh)
    if not 0.0 < thresh < 1.0 or scene_q8(thresh) < 1:          # NaN fails the comparisons
        raise ValueError("scene_cuts threshold %r is outside [1/256, 1)" % (thresh,))
    return SceneCuts(thresh)


def scene_kw(scene_cuts):
    """the keyword `face_detect` and `detect_many` take for `scene_cuts`, checked first: none for None, so the default path is
    called with the same arguments as before the option (as `track.track_kw`)"""
    scene = check_scene(scene_cuts)
    return {} if scene is None else {"scene_cuts": scene}


# ---------------------------------------------------------------- the command line
def scene_arg(text):
    """argparse type of `--scene_cuts`: a fraction in [1/256, 1) (a parse error otherwise)"""
    import argparse
    try:
        return check_scene(float(text)).thresh
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a number in [1/256, 1)" % (text,))


def add_scene_flag(p):
    """`--scene_cuts THRESH` on a command's parser: absent by default (the reference's one take per clip), independent of every
    other flag"""
    p.add_argument('--scene_cuts', default=None, type=scene_arg, metavar='THRESH',
                   help='Split every clip into shots where the colour histogram of a frame differs from the previous frame\'s by more '
                        'than THRESH (in [1/256, 1)) of the largest possible difference, and box, smooth, hold and track every shot on '
                        'its own. No default: 0.3 is a starting point, a choice and not a measured value; fades and dissolves are not '
                        'detected. Default: absent, a clip is one take as in the reference. Not the reference\'s output')


def scene_from_args(a):
    """the `scene_cuts=` of a parsed command line (`add_scene_flag`): None without --scene_cuts, or when the namespace comes from a
    parser without the flag"""
    return check_scene(getattr(a, "scene_cuts", None))


# ---------------------------------------------------------------- the rule on the host
def host_signatures(frames):
    """the signatures of frames uint8 [n,H,W,3] (or a list of [H,W,3] arrays of one shape) on the host: uint32 [n,96]; what
    w2l_frame_hist_rows computes"""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError("host_signatures: frames must be uint8 [n,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    n = len(frames)
    out = np.zeros((n, SIG_WORDS), np.uint32)
    if n and frames[0].size:
        flat = np.ascontiguousarray(frames).reshape(n, -1)
        word = (np.arange(flat.shape[1]) % 3) * SIG_BINS                  # the channel's first word, by the byte's offset
        for i in range(n):
            out[i] = np.bincount(word + (flat[i] >> 3), minlength=SIG_WORDS)
    return out


def _q_and_bound(H, W, q):
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 255:
        raise ValueError("the cut rule's q must be an integer in 1..255, got %r" % (q,))
    if H < 1 or W < 1 or 6 * H * W >= 1 << 31:
        raise ValueError("the cut rule needs H, W >= 1 and 6 * H * W < 2^31, got %d x %d" % (H, W))
    return int(q) * 6 * int(H) * int(W)


def host_cut_flags(sig, H, W, q):
    """the cut rule on the signatures [n,96] of one clip of H x W frames: (cuts int32 [n], dist int64 [n]); what w2l_scene_cuts
    computes for one segment.  Frame 0 is never a cut and has distance 0."""
    bound = _q_and_bound(H, W, q)
    sig = np.asarray(sig).astype(np.int64).reshape(-1, SIG_WORDS)
    dist = np.zeros(len(sig), np.int64)
    if len(sig) > 1:
        dist[1:] = np.abs(sig[1:] - sig[:-1]).sum(axis=1)
    return (dist * 256 > bound).astype(np.int32), dist


def split_shots(n, cuts):
    """[(a, b)] of the shots of a clip of n frames: a new one starts at 0 and at every frame whose cut flag is set (the flag of
    frame 0 is not looked at)"""
    starts = [0] + [i for i in range(1, n) if cuts[i]] if n > 0 else []
    return list(zip(starts, starts[1:] + [n]))


def host_track_shots(cands_per_frame, shots, track):
    """`track.host_track` per shot, a fresh state at every shot's start: a rect tuple or None per frame of the clip"""
    from .track import host_track
    return [r for a, b in shots for r in host_track(cands_per_frame[a:b], track)[0]]


def host_boxes_shots(rects, shots, H, W, pads, T, hold=None):
    """the finish of a clip under the rule, on the host: every shot [a, b) is finished as `many.host_boxes` (strict; a frame without
    a face in any shot is the clip's ValueError) or `many.host_boxes_runs` (with `hold`) finishes a clip of its frames alone.
    Returns (boxes int64 [n,4] of (y1, y2, x1, x2), valid bool [n]); with `shots` = [(0, n)] it is today's finish."""
    from .many import NO_FACE, host_boxes, host_boxes_runs
    if hold is None:
        if any(r is None for r in rects):
            raise ValueError(NO_FACE)
        parts = [(host_boxes(rects[a:b], H, W, pads, T), np.ones(b - a, dtype=bool)) for a, b in shots]
    else:
        parts = [host_boxes_runs(rects[a:b], H, W, pads, T, hold) for a, b in shots]
    if not parts:
        return np.zeros((0, 4), np.int64), np.zeros(0, dtype=bool)
    return np.concatenate([p[0] for p in parts]).astype(np.int64).reshape(-1, 4), np.concatenate([p[1] for p in parts])


# ---------------------------------------------------------------- the device launches
def frame_signatures(frames, sig, offset=0, rows=None):
    """w2l_frame_hist_rows: the signatures of B frames into rows [offset, offset + B) of the int32 arena `sig` [R,96] (the counts
    are below 2^29; the words are the kernel's uint32).  `frames`: one contiguous uint8 device tensor [B,H,W,3], or with `rows` =
    (B, H, W) a device table of B frame addresses - what `s3fd.dense_boxes_rows` takes - read where the frames lie."""
    import torch
    from .._lib import check, current_stream, load, ptr
    if rows is None:
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous() or not frames.is_cuda:
            raise ValueError("frame_signatures: frames must be a contiguous uint8 device tensor [B,H,W,3]")
        B, H, W = (int(v) for v in frames.shape[:3])
        if B < 1:
            return
        table = frames.data_ptr() + np.arange(B, dtype=np.int64) * (H * W * 3)
        frames = torch.from_numpy(table).to(frames.device)       # freed after the launch: the allocator is stream-ordered
    else:
        B, H, W = (int(v) for v in rows)
        if frames.numel() * frames.element_size() < 8 * B:
            raise ValueError("frame_signatures: the address table holds fewer than %d addresses" % B)
    if (sig.dtype != torch.int32 or sig.dim() != 2 or sig.shape[1] != SIG_WORDS or not sig.is_contiguous() or offset < 0
            or offset + B > sig.shape[0]):
        raise ValueError("frame_signatures: an int32 arena [R,%d] with rows [%d, %d) inside it" % (SIG_WORDS, offset, offset + B))
    import ctypes
    check(load().w2l_frame_hist_rows(current_stream(), B, H, W, ptr(frames), ctypes.c_void_p(sig.data_ptr() + 4 * SIG_WORDS * offset)),
          "frame_hist_rows")


def cut_flags(segs, n_seg, sig, q, cuts, status, dist=None):
    """w2l_scene_cuts over a device segment table (BOX_SEGMENT rows, a uint8 or int32 tensor): sig int32 [R,96]
    (`frame_signatures`) -> cuts int32 [R], status int32 [n_seg], and dist int32 [R] if given"""
    import torch
    from .._lib import check, current_stream, load, ptr
    R = int(sig.shape[0])
    for name, t, shape in (("sig", sig, (R, SIG_WORDS)), ("cuts", cuts, (R,)), ("status", status, (n_seg,)), ("dist", dist, (R,))):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError("cut_flags: %s must be a contiguous int32 tensor of shape %s" % (name, shape))
    if segs.numel() * segs.element_size() < n_seg * BOX_SEGMENT.itemsize:
        raise ValueError("cut_flags: the segment table holds fewer than %d segments" % n_seg)
    check(load().w2l_scene_cuts(current_stream(), n_seg, ptr(segs), ptr(sig), R, int(q), ptr(cuts), ptr(dist), ptr(status)), "scene_cuts")


def clip_cuts(sig, H, W, scene):
    """the cut flags of ONE clip whose signatures fill the device arena `sig` [n,96]: one w2l_scene_cuts launch with one segment and
    one small copy back -> (cuts int32 [n], dist int32 [n]) as numpy arrays"""
    import torch
    n = int(sig.shape[0])
    seg = np.zeros(1, dtype=BOX_SEGMENT)
    seg[0] = (0, n, H, W)
    segs = torch.from_numpy(seg.view(np.uint8)).to(sig.device)
    out = torch.empty(2 * n + 1, dtype=torch.int32, device=sig.device)       # cuts [n], dist [n], status [1]
    cut_flags(segs, 1, sig, scene_q8(scene.thresh), out[:n], out[2 * n:], dist=out[n:2 * n])
    res = out.cpu().numpy()
    if res[2 * n] != 0:
        raise AssertionError("w2l_scene_cuts did not follow the clip's segment (status %d)" % res[2 * n])
    return res[:n], res[n:2 * n]


MAX_UPLOAD_BYTES = 256 << 20     # frames `distances` uploads at a time


def distances(frames, device=None):
    """D(i) / (6 * H * W) per frame of a video, float64 [n] in [0, 1] with 0 for frame 0: what a threshold is compared against
    (frame i starts a new shot iff the quantised rule fires, about distances(frames)[i] > thresh).  `frames`: a uint8 device tensor
    [n,H,W,3] - the two kernels; or host frames [n,H,W,3] - uploaded to `device` in pieces for the kernels, or with `device` None
    the host statements."""
    import torch
    if not isinstance(frames, torch.Tensor):
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
            raise ValueError("distances: frames must be uint8 [n,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    n, H, W = (int(v) for v in frames.shape[:3])
    if n == 0:
        return np.zeros(0, np.float64)
    _q_and_bound(H, W, 1)
    if not isinstance(frames, torch.Tensor) and device is None:
        return host_cut_flags(host_signatures(frames), H, W, 1)[1] / float(6 * H * W)
    dev = frames.device if isinstance(frames, torch.Tensor) else torch.device(device)
    sig = torch.empty((n, SIG_WORDS), dtype=torch.int32, device=dev)
    step = max(1, MAX_UPLOAD_BYTES // (H * W * 3))
    for lo in range(0, n, step):
        piece = frames[lo:lo + step]
        frame_signatures(piece.contiguous() if isinstance(piece, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(piece)).to(dev),
                         sig, lo)
    return clip_cuts(sig, H, W, SceneCuts(1 / 256))[1].astype(np.float64) / float(6 * H * W)


def main(argv=None):
    """`python -m wav2lip_amd.face_detection.scene VIDEO.avi [--scene_cuts T]`: the per-frame distance of an AVI file (uncompressed
    or Motion-JPEG, `container.read_avi`), and with a threshold the frames that start a shot"""
    import argparse
    from ..container import read_avi
    p = argparse.ArgumentParser(description="Per-frame scene-cut distance D / (6 H W) of a video, to choose --scene_cuts by")
    p.add_argument("video", help="an AVI file (uncompressed 24-bit or Motion-JPEG)")
    add_scene_flag(p)
    p.add_argument("--host", default=False, action="store_true", help="compute on the host instead of the GPU")
    a = p.parse_args(argv)
    scene = scene_from_args(a)
    frames = read_avi(a.video)["frames"]
    d = distances(frames, device=None if a.host else "cuda")
    H, W = frames.shape[1:3]
    cuts = None if scene is None else (np.round(d * (6 * H * W)).astype(np.int64) * 256 > scene_q8(scene.thresh) * 6 * H * W)
    for i, v in enumerate(d):
        print("%6d  %.6f%s" % (i, v, "  cut" if cuts is not None and cuts[i] else ""))
    if cuts is not None:
        print("cuts at frames: %s" % (" ".join(str(i) for i in np.flatnonzero(cuts)) or "none"))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
