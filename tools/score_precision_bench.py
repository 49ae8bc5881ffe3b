"""fp32 against bf16 SyncNet scoring, alternated in one process: windows/s of `evaluation.lse_many` in each precision over the same
seeded clips.

    python tools/score_precision_bench.py [--clips 200] [--alternations 5] [--batch 128] [--min-seconds 1.0] [--seed 0]

The clips, their 96x96 face crops and their mel spectrograms are those of tools/score_bench.py, made once before any timing and
kept on the device.  Each precision owns a SyncNet (SyncNet_color keeps one inference graph, so one model would rebuild its
graph at every switch); both are warmed with one full pass first.  A sample repeats whole `lse_many` passes - crops and mel in,
every clip's scores on the host out - until at least --min-seconds have passed; samples of fp32 and bf16 alternate,
--alternations pairs.  Prints one JSON line: per precision the windows/s of every sample, median, min and max (the spread), the
bf16 / fp32 ratio of the medians, the kernel families of the bf16 plan's launches (`dispatch()`), and for the last pass of each the
largest |d LSE-D| and |d LSE-C| over the clips and the number of clips whose offset differs.

The per-kernel table comes from one separate run under the profiler:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/score_precision_bench.py --alternations 1"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filelist_bench import make_clips  # noqa: E402
from score_bench import model, prepare  # noqa: E402
from wav2lip_amd import evaluation  # noqa: E402


def one_pass(S, data, batch, precision):
    res = evaluation.lse_many(S, (evaluation.ScoreJob(i, f, m) for i, (f, m) in enumerate(data)), batch_size=batch,
                              precision=precision)
    torch.cuda.synchronize()
    return res


def sample(S, data, batch, precision, min_s):
    """whole passes until >= min_s seconds; returns (windows/s, the last pass's results)"""
    windows, t0 = 0, time.perf_counter()
    while True:
        res = one_pass(S, data, batch, precision)
        windows += sum(r["n"] for r in res)
        t = time.perf_counter() - t0
        if t >= min_s:
            return windows / t, res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if a.alternations < 1 or a.min_seconds <= 0:
        ap.error("--alternations >= 1 and --min-seconds > 0")
    dev = torch.device("cuda", 0)
    data = prepare(make_clips(a.clips, a.seed), dev)
    nets = {p: model(dev) for p in ("f32", "bf16")}
    last = {}
    for p, S in nets.items():             # each model builds its plan (and split-K scratch) before anything is timed
        last[p] = one_pass(S, data, a.batch, p)
    wps = {p: [] for p in nets}
    for _ in range(a.alternations):
        for p, S in nets.items():
            w, last[p] = sample(S, data, a.batch, p, a.min_seconds)
            wps[p].append(w)
            print("%s: %.1f windows/s" % (p, w), file=sys.stderr, flush=True)
    out = {"clips": a.clips, "windows": sum(r["n"] for r in last["f32"]), "batch": a.batch, "alternations": a.alternations,
           "min_seconds": a.min_seconds, "device": torch.cuda.get_device_name(dev)}
    for p, v in wps.items():
        out[p] = {"windows_per_s": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1),
                  "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}
    out["speedup_median"] = round(out["bf16"]["median"] / out["f32"]["median"], 3)
    out["speedup_range"] = [round(out["bf16"]["min"] / out["f32"]["max"], 3), round(out["bf16"]["max"] / out["f32"]["min"], 3)]
    graph = next(iter(nets["bf16"]._graphs.values()))[1]
    fams = {}
    for _, fam, tile, ks in graph.dispatch():
        key = "%s tile %d ksplit %d" % (fam, tile, ks)
        fams[key] = fams.get(key, 0) + 1
    out["bf16_dispatch"] = fams
    pairs = [(x, y) for x, y in zip(last["bf16"], last["f32"]) if x["n"]]
    assert all(x["key"] == y["key"] and x["n"] == y["n"] for x, y in zip(last["bf16"], last["f32"]))
    out["bf16_vs_f32"] = {"max_abs_d_lse_d": round(max(abs(x["lse_d"] - y["lse_d"]) for x, y in pairs), 6),
                          "max_abs_d_lse_c": round(max(abs(x["lse_c"] - y["lse_c"]) for x, y in pairs), 6),
                          "offsets_differ": sum(x["offset"] != y["offset"] for x, y in pairs), "clips_scored": len(pairs)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
