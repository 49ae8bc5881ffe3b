#!/usr/bin/env python
"""Motion-JPEG video in and out on one MI355X, in ONE process, every figure the median and the range of --alternations timed
passes (at least five) that alternate between the paths compared, after a warm-up pass of each:
  1. the encoder alone, frames/s at 480x640 and 720x1280: `jpeg.encode_frames` on frames that lie on the device (staging, two
     kernels, the lengths and the files' bytes back) against a PIL loop on one thread with the same quality, 4:2:0 and
     restart_marker_rows (frames in host memory); whether the bytes are equal;
  2. the decoder alone on those files: `jpeg.decode_frames` at restart_rows=1 (one lane per interval) against the same frames
     written WITHOUT restarts (one lane per file: the path `jpeg.decode_files` has) and against a PIL loop; the share of
     decode_frames' time spent in the host's parse + marker scan (timed on its own over the same files);
  3. `inference.main` end to end on one synthetic clip, --out_codec raw against mjpg (a random-weight generator, --box: no
     detector), with the two files' sizes.
Synthetic frames: a smooth colour field with mild sensor noise (tools/clipstore_bench.py's), so the files have a camera
frame's size rather than noise's.  Prints one JSON line.
    python tools/video_io_bench.py [--frames 16] [--alternations 5] [--clip_frames 50] [--skip_inference]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def frame(rng, h, w):
    """uint8 [h,w,3]: a coarse random grid interpolated up, plus noise of sigma 4"""
    from PIL import Image
    g = Image.fromarray(rng.integers(30, 226, (9, 12, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
    return np.clip(np.asarray(g) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def summary(res, key, rates):
    res[key + "_per_s"] = [round(x, 1) for x in rates]
    res[key + "_median"] = round(float(np.median(rates)), 1)
    res[key + "_range"] = [round(min(rates), 1), round(max(rates), 1)]


def alternate(paths, n_items, passes):
    """{name: [items/s per pass]}: a warm-up of each path, then `passes` rounds that run every path once"""
    for f in paths.values():
        f()
    rates = {k: [] for k in paths}
    for _ in range(passes):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            rates[k].append(n_items / (time.perf_counter() - t0))
    return rates


def pil_encode(bgr, quality, rows):
    from PIL import Image
    buf = io.BytesIO()
    kw = {} if rows is None else {"restart_marker_rows": rows}
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality, subsampling=2, **kw)
    return buf.getvalue()


def pil_decode(d):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1]


def codec_bench(res, dev, h, w, n, passes, quality=95):
    from wav2lip_amd import jpeg
    tag = "%dx%d" % (h, w)
    rng = np.random.default_rng(h)
    host = np.stack([frame(rng, h, w) for _ in range(n)])
    frames = torch.from_numpy(host).to(dev)
    files = jpeg.encode_frames(frames, quality=quality, restart_rows=1)
    plain = [pil_encode(f, quality, None) for f in host]
    res[tag + "_encoder_same_bytes"] = files == [pil_encode(f, quality, 1) for f in host]
    res[tag + "_file_bytes_mean"] = round(sum(map(len, files)) / n, 1)
    res[tag + "_raw_over_file"] = round(h * w * 3 * n / sum(map(len, files)), 2)
    rates = alternate({"pil": lambda: [pil_encode(f, quality, 1) for f in host],
                       "device": lambda: jpeg.encode_frames(frames, quality=quality, restart_rows=1)}, n, passes)
    for k in rates:
        summary(res, tag + "_encode_" + k, rates[k])
    res[tag + "_encode_device_over_pil"] = round(res[tag + "_encode_device_median"] / res[tag + "_encode_pil_median"], 3)

    def scan():
        for d in files:
            info, ri = jpeg.parse_frame(d)
            jpeg.restart_segments(d, info, ri)
    got = jpeg.decode_frames(files, dev)
    res[tag + "_decoder_same_images"] = (all(np.array_equal(g.cpu().numpy(), pil_decode(d)) for g, d in zip(got, files)) and
                                         all(np.array_equal(g.cpu().numpy(), pil_decode(d))
                                             for g, d in zip(jpeg.decode_frames(plain, dev), plain)))
    del got
    rates = alternate({"pil": lambda: [pil_decode(d) for d in files],
                       "device_restart_rows_1": lambda: jpeg.decode_frames(files, dev),
                       "device_no_restarts": lambda: jpeg.decode_frames(plain, dev),
                       "host_scan_alone": scan}, n, passes)
    for k in rates:
        summary(res, tag + "_decode_" + k, rates[k])
    res[tag + "_decode_device_over_pil"] = round(res[tag + "_decode_device_restart_rows_1_median"] / res[tag + "_decode_pil_median"], 3)
    res[tag + "_decode_restarts_over_none"] = round(res[tag + "_decode_device_restart_rows_1_median"] /
                                                    res[tag + "_decode_device_no_restarts_median"], 3)
    res[tag + "_host_scan_share"] = round(res[tag + "_decode_device_restart_rows_1_median"] / res[tag + "_decode_host_scan_alone_median"], 3)


def inference_bench(res, dev, clip_frames, passes):
    from scipy.io import wavfile
    from wav2lip_amd import container, inference, models, synthetic as synth
    h, w = 480, 640
    rng = np.random.default_rng(5)
    base = frame(rng, h, w + 2 * clip_frames)
    clip = np.stack([base[:, 2 * k:2 * k + w] for k in range(clip_frames)])
    with tempfile.TemporaryDirectory() as tmp:
        container.write_avi(os.path.join(tmp, "face.avi"), clip, 25)
        wavfile.write(os.path.join(tmp, "a.wav"), 16000, np.clip(np.round(synth.noise_wav(16000 * clip_frames // 25, seed=3) * 32768.0), -32768, 32767).astype(np.int16))
        sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)
        torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer": None, "global_step": 0, "global_epoch": 0},
                   os.path.join(tmp, "ckpt.pth"))
        outs = {c: os.path.join(tmp, c + ".avi") for c in ("raw", "mjpg")}

        def run(codec):
            inference.main(["--checkpoint_path", os.path.join(tmp, "ckpt.pth"), "--face", os.path.join(tmp, "face.avi"), "--audio",
                            os.path.join(tmp, "a.wav"), "--box", "100", "380", "180", "460", "--outfile", outs[codec], "--out_codec", codec],
                           keep_frames=False)
        n = None
        rates = alternate({c: (lambda c=c: run(c)) for c in outs}, 1, passes)
        n = len(container.read_avi(outs["raw"])["frames"])
        res["inference_frames"], res["inference_size"] = n, "%dx%d" % (h, w)
        for c in outs:
            summary(res, "inference_" + c + "_frames", [r * n for r in rates[c]])
            res["inference_" + c + "_file_bytes"] = os.path.getsize(outs[c])
        res["inference_mjpg_over_raw"] = round(res["inference_mjpg_frames_median"] / res["inference_raw_frames_median"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16, help="frames of one encoder / decoder pass")
    ap.add_argument("--alternations", type=int, default=5, help="timed passes of each path (at least 5)")
    ap.add_argument("--clip_frames", type=int, default=50, help="frames (and 1/25 s of audio each) of the inference clip")
    ap.add_argument("--skip_inference", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "video_io_bench needs a HIP device"
    dev = torch.device("cuda:0")
    passes = max(5, a.alternations)
    res = {"frames": a.frames, "alternations": passes, "lib": os.path.basename(os.environ.get("W2L_HIP_LIB", "")) or "default"}
    for h, w in ((480, 640), (720, 1280)):
        codec_bench(res, dev, h, w, a.frames, passes)
    if not a.skip_inference:
        inference_bench(res, dev, a.clip_frames, passes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
