#!/usr/bin/env python
"""Loading the training set on one MI355X: a synthetic directory in the layout `preprocess` writes - clips of 30-120 face crops
whose sides run from about 90 to 220 pixels, written by PIL at quality 95, 4:2:0, plus a short audio.wav each - then in ONE process
  1. end to end: files/s of `ClipStore.from_directory` with decode="host" (PIL per file, one upload and one resize launch per
     frame: the code before the device decoder, unchanged) and with decode="device", alternated --alternations times each (at
     least five) after a warm-up load of each; median and range of both, and whether the two stores hold the same bytes;
  2. the decoder alone, on the same files' bytes held in host memory, alternating per sample: files/s of `jpeg.decode_files` in
     batches of ClipStore.DEVICE_BATCH_FILES (parsing, staging, one copy in, the kernels, the status back; the images stay on the
     device) against a PIL loop on one thread (the images in host memory), median and range of each, and whether a sample of
     the images is equal.
Prints one JSON line.
    python tools/clipstore_bench.py [--clips 200] [--alternations 5] [--samples 5] [--seed 0]"""
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


_noise = {}


def crop(rng, h, w):
    """a face-like crop: a smooth colour field (a coarse random grid, interpolated) with mild sensor noise, uint8 [h,w,3] RGB"""
    from PIL import Image
    if not _noise:
        _noise[0] = np.random.default_rng(1).normal(0, 4, (256, 256, 3))
    g = Image.fromarray(rng.integers(30, 226, (6, 6, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
    y, x = int(rng.integers(0, 256 - h + 1)), int(rng.integers(0, 256 - w + 1))
    return np.clip(np.asarray(g) + _noise[0][y:y + h, x:x + w], 0, 255).astype(np.uint8)


def write_tree(root, lists, clips, seed):
    """the directory and filelists/train.txt; returns the number of files"""
    from PIL import Image
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    os.makedirs(lists)
    n = 0
    with open(os.path.join(lists, "train.txt"), "w") as fh:
        for c in range(clips):
            rel = "spk%d/%05d" % (c % 7, c)
            d = os.path.join(root, rel)
            os.makedirs(d)
            frames = int(rng.integers(30, 121))
            side = int(rng.integers(90, 221))                 # a clip's crops follow one face: sizes wander around one side
            for i in range(frames):
                h, w = (int(np.clip(side + rng.integers(-8, 9), 90, 220)) for _ in range(2))
                Image.fromarray(crop(rng, h, w)).save(os.path.join(d, "%d.jpg" % i), format="JPEG", quality=95, subsampling=2)
            wavfile.write(os.path.join(d, "audio.wav"), 16000, (rng.normal(0, 3000, frames * 640)).astype(np.int16))
            fh.write(rel + "\n")
            n += frames
    return n


def summary(res, key, rates):
    res[key + "_files_per_s"] = [round(x, 1) for x in rates]
    res[key + "_median"] = round(float(np.median(rates)), 1)
    res[key + "_range"] = [round(min(rates), 1), round(max(rates), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=5, help="timed loads of each mode (at least 5)")
    ap.add_argument("--samples", type=int, default=5, help="timed passes of the decoder alone, each path (at least 5)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from PIL import Image
    from wav2lip_amd import data, jpeg
    assert torch.cuda.is_available(), "clipstore_bench needs a HIP device"
    dev = torch.device("cuda:0")
    res = {"clips": a.clips}
    with tempfile.TemporaryDirectory() as tmp:
        root, lists = os.path.join(tmp, "data"), os.path.join(tmp, "filelists")
        n = write_tree(root, lists, a.clips, a.seed)
        res["files"] = n
        datas = []
        for d, _, fs in sorted(os.walk(root)):
            datas += [open(os.path.join(d, f), "rb").read() for f in sorted(fs) if f.endswith(".jpg")]
        res["file_bytes_mean"] = round(sum(len(d) for d in datas) / len(datas), 1)

        def load(mode):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = data.ClipStore.from_directory(root, "train", dev, filelist_dir=lists, decode=mode)
            store.frames()
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0), store

        modes = ("host", "device")
        stores = {m: load(m)[1] for m in modes}               # warm-up (code objects, the allocator, the page cache) and the comparison
        res["same_store"] = bool(torch.equal(stores["host"].frames(), stores["device"].frames())
                                 and torch.equal(stores["host"].mels._bank(), stores["device"].mels._bank())
                                 and stores["host"].row_of == stores["device"].row_of)
        res["host_decoded"] = stores["device"].host_decoded
        del stores
        rates = {m: [] for m in modes}
        for _ in range(max(5, a.alternations)):
            for m in modes:
                rates[m].append(load(m)[0])
        for m in modes:
            summary(res, "load_" + m, rates[m])
        res["load_device_over_host"] = round(res["load_device_median"] / res["load_host_median"], 3)

    # the decoder alone
    cap = data.ClipStore.DEVICE_BATCH_FILES

    def device():
        out = []
        for i in range(0, len(datas), cap):
            out += jpeg.decode_files(datas[i:i + cap], dev)
        return out

    def pil():
        return [np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1] for d in datas]
    paths = {"pil": pil, "device": device}
    outs = {k: f() for k, f in paths.items()}                 # warm-up, and the images to compare
    pick = range(0, len(datas), max(1, len(datas) // 64))
    res["decoder_same_images"] = all(np.array_equal(outs["pil"][i], outs["device"][i].cpu().numpy()) for i in pick)
    del outs
    rates = {k: [] for k in paths}
    for _ in range(max(5, a.samples)):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            rates[k].append(len(datas) / (time.perf_counter() - t0))
    for k in paths:
        summary(res, "decoder_" + k, rates[k])
    res["decoder_device_over_pil"] = round(res["decoder_device_median"] / res["decoder_pil_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
