"""Streaming lip-sync in shared batches against the per-stream loop, alternated in one process.

    python tools/stream_bench.py [--streams 1 8 64 256] [--ticks 250 250 80 40] [--paced_ticks 100 100 80 40] [--alternations 5]
                                 [--paced_alternations 5] [--batch 128]

The defaults are the sweep EXPERIMENTS.md reports: one JSON line per stream count (--ticks / --paced_ticks give one value per
stream count, or one for all; fewer ticks at large S keep the per-stream loop's pass short).

S synthetic 25 fps streams of 160x160 frames with a fixed 110x110 face box, audio in 40 ms ticks (640 samples: one row per
stream per tick once the first window is there).  Two loops over the same seeded audio, each on a model of its own:

  shared      `streaming.LipsyncStreams`: per tick `feed` every stream, one `step(flush=True)`; frames arrive through the sink
  per_stream  what the public API offered before: per stream per tick `audio.melspectrogram_device` on the trailing samples
              (from three columns before the first window wanted, so that the columns used are exact) and
              `Wav2LipRunner.run_frames` on that stream's ready rows, frames copied to the host

(a) un-paced: ticks as fast as the loop goes; frames/s, and streams held in real time = frames/s / 25.
(b) paced: tick k is fed at k * 40 ms (a loop that cannot keep up falls behind and its latency grows); per row the time from the
    `feed` that completed it to the delivery of its frame; p50 / p99 over all rows.  While it waits for the next tick the shared
    loop polls `step()` (nothing new to compute: it only delivers what has finished).
Pass 0 of each loop is its warm-up (plans built) and is not reported.  Then the loops alternate.  Prints one JSON line.

    python tools/stream_bench.py --live_video [--streams 8] [--ticks 100] [--alternations 5]

compares, on S copies of a seeded 160x160 video whose faces the seeded S3FD finds (one frame and 40 ms of audio per tick):

  upfront  what `python -m wav2lip_amd.streaming` does without `--live_video`: `inference.face_detect` over every frame of every
           video, one clip after another, then the streams opened with frames and boxes and fed tick by tick
  live     `open_live`: per tick `feed` + `feed_frames` of every stream and one `step(flush=True)`; detection runs as frames arrive

frames/s over the whole pass (detection included on both sides), and per row the number of ticks between the tick whose audio
completed it and the tick in which its frame was delivered: the lag live detection adds is T - 1 frames plus one tick by
construction, and this is what is measured of it.

    python tools/stream_bench.py --sample_rate 48000 [--streams 64] [--ticks 80] [--alternations 5]

compares S streams opened at that rate and fed 40 ms of it per tick (converted to 16 kHz on the device as they stream, one
w2l_resample_stream launch per tick) with the same streams fed the same audio converted beforehand, outside the timed loop:
frames/s, and the wall time per tick over the whole pass."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wav2lip_amd import audio, inference, models, streaming  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402

BOX = (30, 140, 25, 135)
TICK = 640


def model(dev):
    G = models.Wav2Lip()
    G.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0))
    return G.to(dev).eval()


def ready_ticks(ticks):
    """tick after whose feed row i is complete (the last row, the tail window, with the close at the last tick)"""
    out, i = [], 0
    for t in range(ticks):
        final = streaming.final_columns((t + 1) * TICK, t == ticks - 1)
        while streaming.row_start(i, 25.) + 16 <= final:
            out.append(t)
            i += 1
    return out + [ticks - 1]


class Clock:
    """feed times per tick and delivery latencies per row"""

    def __init__(self, ticks, pace):
        self.ready, self.fed, self.lat, self.count, self.pace, self.t0 = ready_ticks(ticks), [0.0] * ticks, [], {}, pace, None

    def wait(self, t, poll=None):
        if self.t0 is None:
            self.t0 = time.perf_counter()
        if self.pace:
            while time.perf_counter() < self.t0 + t * 0.040:
                if poll is not None:
                    poll()
                time.sleep(0.0005)
        self.fed[t] = time.perf_counter()

    def sink(self, key, frame):
        if frame is not None:
            i = self.count.get(key, 0)
            self.count[key] = i + 1
            self.lat.append(time.perf_counter() - self.fed[self.ready[i]])


def run_shared(G, wavs, frames, ticks, batch, dev, pace):
    clock = Clock(ticks, pace)
    ls = streaming.LipsyncStreams(G, batch_size=batch, sink=clock.sink)
    for k in range(len(wavs)):
        ls.open(k, frames, [BOX] * len(frames))
    t_start = time.perf_counter()
    for t in range(ticks):
        clock.wait(t, ls.step)
        for k, w in enumerate(wavs):
            ls.feed(k, w[t * TICK:(t + 1) * TICK])
            if t == ticks - 1:
                ls.close(k)
        ls.step(flush=True)
    ls.drain()
    torch.cuda.synchronize()
    return clock, time.perf_counter() - t_start


def run_per_stream(G, wavs, frames, ticks, batch, dev, pace):
    clock = Clock(ticks, pace)
    runner = inference.Wav2LipRunner(G, batch)
    frames_dev = torch.from_numpy(np.stack(frames)).to(dev)
    state = [dict(held=np.empty(0, np.float32), first=0, n=0, row=0) for _ in wavs]
    t_start = time.perf_counter()
    for t in range(ticks):
        clock.wait(t)
        closed = t == ticks - 1
        for k, w in enumerate(wavs):
            s = state[k]
            s["held"] = np.concatenate([s["held"], w[t * TICK:(t + 1) * TICK]])
            s["n"] += TICK
            final = streaming.final_columns(s["n"], closed)
            starts = []
            while streaming.row_start(s["row"] + len(starts), 25.) + 16 <= final:
                starts.append(streaming.row_start(s["row"] + len(starts), 25.))
            if closed:
                starts.append(final - 16)
            if not starts:
                continue
            s0 = max(0, (starts[0] - 3) * 200)                       # columns >= s0/200 + 3 of the trailing signal are exact
            mel = audio.melspectrogram_device(s["held"][s0 - s["first"]:], dev)
            rel = torch.tensor([c - s0 // 200 for c in starts], dtype=torch.int32, device=dev)
            idx = [(s["row"] + j) % len(frames) for j in range(len(starts))]
            out = runner.run_frames(frames_dev, idx, [BOX] * len(starts), mel=mel, starts=rel).cpu().numpy()
            for f in out:
                clock.sink(k, f)
            s["row"] += len(starts)
            s["held"], s["first"] = s["held"][s0 - s["first"]:], s0
    torch.cuda.synchronize()
    return clock, time.perf_counter() - t_start


def live_clip(ticks):
    frames = synth.filelist_clips()["c3"][0]                  # 160x160, a face in every frame
    return np.stack([frames[k % len(frames)] for k in range(ticks)])


class TickClock:
    """per row: ticks between the tick that completed its audio and the tick of its delivery"""

    def __init__(self, ticks):
        self.ready, self.count, self.lag, self.tick = ready_ticks(ticks), {}, [], 0

    def sink(self, key, frame):
        if frame is not None:
            i = self.count.get(key, 0)
            self.count[key] = i + 1
            self.lag.append(self.tick - self.ready[i])


def run_upfront(G, det, video, wavs, ticks, batch):
    clock = TickClock(ticks)
    t_start = time.perf_counter()
    boxes = [[c for _, c in inference.face_detect(list(video), detector=det, pads=[0, 10, 0, 0], nosmooth=False, batch_size=16)]
             for _ in wavs]
    ls = streaming.LipsyncStreams(G, batch_size=batch, sink=clock.sink)
    for k in range(len(wavs)):
        ls.open(k, list(video), boxes[k])
    for t in range(ticks):
        clock.tick = t
        for k, w in enumerate(wavs):
            ls.feed(k, w[t * TICK:(t + 1) * TICK])
            if t == ticks - 1:
                ls.close(k)
        ls.step(flush=True)
    clock.tick = ticks
    ls.drain()
    torch.cuda.synchronize()
    return clock, time.perf_counter() - t_start


def run_live(G, det, video, wavs, ticks, batch):
    clock = TickClock(ticks)
    t_start = time.perf_counter()
    ls = streaming.LipsyncStreams(G, batch_size=batch, sink=clock.sink, detector=det, pads=(0, 10, 0, 0), smooth_T=5,
                                  face_det_batch_size=16)
    for k in range(len(wavs)):
        ls.open_live(k)
    for t in range(ticks):
        clock.tick = t
        for k, w in enumerate(wavs):
            ls.feed(k, w[t * TICK:(t + 1) * TICK])
            ls.feed_frames(k, [video[t]])
            if t == ticks - 1:
                ls.close_video(k)
                ls.close(k)
        ls.step(flush=True)
    clock.tick = ticks
    ls.drain()
    torch.cuda.synchronize()
    if ls.errors:
        raise SystemExit("live detection ended streams: %s" % ls.errors)
    return clock, time.perf_counter() - t_start


def bench_live(S, ticks, a, dev):
    from wav2lip_amd import face_detection
    det = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(dev),
                                       state_dict=synth.s3fd_state_dict())
    video = live_clip(ticks)
    wavs = [synth.noise_wav(ticks * TICK, seed=a.seed * 100003 + k) for k in range(S)]
    loops = {"upfront": (run_upfront, model(dev)), "live": (run_live, model(dev))}
    res = {k: {"fps": [], "lag_ticks_median": [], "lag_ticks_max": []} for k in loops}
    for name, (fn, G) in loops.items():                   # pass 0: warm-up, plans and detector graphs built
        clock, t = fn(G, det, video, wavs, ticks, a.batch)
        res[name].update(frames=len(clock.lag), first_pass_s=round(t, 2))
    for _ in range(a.alternations):
        for name, (fn, G) in loops.items():
            clock, t = fn(G, det, video, wavs, ticks, a.batch)
            res[name]["fps"].append(len(clock.lag) / t)
            res[name]["lag_ticks_median"].append(float(np.median(clock.lag)))
            res[name]["lag_ticks_max"].append(float(max(clock.lag)))
    for name in loops:
        for key in ("fps", "lag_ticks_median", "lag_ticks_max"):
            res[name][key] = stats(res[name][key])
    out = {"mode": "live_video", "streams": S, "ticks": ticks, "batch": a.batch, "alternations": a.alternations}
    out.update(res)
    out["live_over_upfront_median"] = round(res["live"]["fps"]["median"] / res["upfront"]["fps"]["median"], 3)
    out["apart_by_more_than_the_spread"] = bool(res["live"]["fps"]["min"] > res["upfront"]["fps"]["max"]
                                                or res["live"]["fps"]["max"] < res["upfront"]["fps"]["min"])
    out["added_lag_ticks_median"] = round(res["live"]["lag_ticks_median"]["median"] - res["upfront"]["lag_ticks_median"]["median"], 1)
    return out


def run_rate(G, wavs, frames, ticks, batch, rate):
    """S streams opened at `rate`, each fed a 40 ms slice per tick (the rest with the last), one `step(flush=True)` per tick"""
    n, tick = [0], int(rate * 0.040)
    ls = streaming.LipsyncStreams(G, batch_size=batch, sink=lambda key, frame: n.__setitem__(0, n[0] + (frame is not None)))
    for k in range(len(wavs)):
        ls.open(k, frames, [BOX] * len(frames), sample_rate=rate)
    per_tick = []
    t_start = time.perf_counter()
    for t in range(ticks):
        t0 = time.perf_counter()
        for k, w in enumerate(wavs):
            ls.feed(k, w[t * tick:] if t == ticks - 1 else w[t * tick:(t + 1) * tick])
            if t == ticks - 1:
                ls.close(k)
        ls.step(flush=True)
        per_tick.append(time.perf_counter() - t0)
    ls.drain()
    torch.cuda.synchronize()
    return n[0], time.perf_counter() - t_start, per_tick, ls.resample_launches


def bench_rate(S, ticks, a, dev):
    """streams fed at --sample_rate (converted on the device as they stream) against the same streams fed the same audio
    converted to 16 kHz beforehand (`audio.resample` of the whole signal, outside the timed loop)"""
    rate = a.sample_rate
    r = np.random.default_rng(a.seed)
    frames = list(r.integers(0, 256, (16, 160, 160, 3), dtype=np.uint8))
    src = [synth.noise_wav(ticks * int(rate * 0.040), seed=a.seed * 100003 + k) for k in range(S)]
    pre = [audio.resample(w, rate, 16000) for w in src]
    loops = {"native": (model(dev), src, rate), "pre16": (model(dev), pre, 16000)}
    res = {k: {"fps": [], "tick_ms": [], "step_host_ms_median": []} for k in loops}
    for name, (G, wavs, rt) in loops.items():              # pass 0: warm-up, plans built, filter tables uploaded
        n, t, _, launches = run_rate(G, wavs, frames, ticks, a.batch, rt)
        res[name].update(frames=n, first_pass_s=round(t, 2), resample_launches=launches)
    for _ in range(a.alternations):
        for name, (G, wavs, rt) in loops.items():
            n, t, per_tick, _ = run_rate(G, wavs, frames, ticks, a.batch, rt)
            res[name]["fps"].append(n / t)
            res[name]["tick_ms"].append(1e3 * t / ticks)                 # the whole pass, drain and synchronize included
            res[name]["step_host_ms_median"].append(1e3 * float(np.median(per_tick)))
    for name in loops:
        for key in ("fps", "tick_ms", "step_host_ms_median"):
            res[name][key] = stats(res[name][key], 1 if key == "fps" else 3)
    out = {"mode": "sample_rate", "sample_rate": rate, "streams": S, "ticks": ticks, "batch": a.batch, "alternations": a.alternations,
           "outputs_per_tick": S * 640}
    out.update(res)
    out["native_over_pre16_median"] = round(res["native"]["fps"]["median"] / res["pre16"]["fps"]["median"], 3)
    out["added_tick_ms_median"] = round(res["native"]["tick_ms"]["median"] - res["pre16"]["tick_ms"]["median"], 3)
    out["apart_by_more_than_the_spread"] = bool(res["native"]["fps"]["max"] < res["pre16"]["fps"]["min"]
                                                or res["native"]["fps"]["min"] > res["pre16"]["fps"]["max"])
    return out


def stats(v, nd=1):
    return {"samples": [round(x, nd) for x in v], "median": round(float(np.median(v)), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def bench_one(S, ticks, paced_ticks, a, dev):
    r = np.random.default_rng(a.seed)
    frames = list(r.integers(0, 256, (16, 160, 160, 3), dtype=np.uint8))
    wavs = [synth.noise_wav(max(ticks, paced_ticks) * TICK, seed=a.seed * 100003 + k) for k in range(S)]
    loops = {"shared": (run_shared, model(dev)), "per_stream": (run_per_stream, model(dev))}
    out = {"streams": S, "ticks": ticks, "batch": a.batch, "alternations": a.alternations,
           "paced_ticks": paced_ticks, "paced_alternations": a.paced_alternations}
    res = {k: {"fps": [], "p50_ms": [], "p99_ms": [], "paced_behind_s": []} for k in loops}
    for name, (fn, G) in loops.items():                   # pass 0: warm-up, plans built
        clock, t = fn(G, wavs, frames, ticks, a.batch, dev, False)
        res[name].update(frames=len(clock.lat), first_pass_s=round(t, 2))
    for _ in range(a.alternations):
        for name, (fn, G) in loops.items():
            clock, t = fn(G, wavs, frames, ticks, a.batch, dev, False)
            res[name]["fps"].append(len(clock.lat) / t)
    for _ in range(a.paced_alternations):
        for name, (fn, G) in loops.items():
            clock, t = fn(G, wavs, frames, paced_ticks, a.batch, dev, True)
            lat = np.array(clock.lat) * 1e3
            res[name]["p50_ms"].append(float(np.percentile(lat, 50)))
            res[name]["p99_ms"].append(float(np.percentile(lat, 99)))
            res[name]["paced_behind_s"].append(t - paced_ticks * 0.040)        # well above one tick: the loop did not keep up
    for name in loops:
        x = res[name]
        x["plans"] = sorted({k[0] for k in loops[name][1]._graphs})
        x["fps"] = stats(x["fps"])
        x["realtime_streams"] = round(x["fps"]["median"] / 25., 1)
        for key in ("p50_ms", "p99_ms", "paced_behind_s"):
            x[key] = stats(x[key], 2) if x[key] else None
    out.update(res)
    out["shared_over_per_stream_median"] = round(res["shared"]["fps"]["median"] / res["per_stream"]["fps"]["median"], 3)
    out["ahead_by_more_than_the_spread"] = bool(res["shared"]["fps"]["min"] > res["per_stream"]["fps"]["max"])
    if a.paced_alternations:                              # the same verdict for the paced latencies: lower is better
        for key in ("p50_ms", "p99_ms"):
            out["paced_%s_lower_by_more_than_the_spread" % key[:3]] = bool(res["shared"][key]["max"] < res["per_stream"][key]["min"])
    return out


def per_count(values, n, name):
    if len(values) not in (1, n):
        raise SystemExit("--%s takes one value, or one per stream count" % name)
    return values * n if len(values) == 1 else values


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--ticks", type=int, nargs="+", default=[250, 250, 80, 40])
    ap.add_argument("--paced_ticks", type=int, nargs="+", default=[100, 100, 80, 40])
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--paced_alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--live_video", action="store_true", help="live face detection against detection up front (see the module text)")
    ap.add_argument("--sample_rate", type=int, default=16000,
                    help="other than 16000: streams fed at this rate against the same streams fed audio converted beforehand")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    if a.sample_rate != 16000:
        for S, t in zip(a.streams, per_count(a.ticks, len(a.streams), "ticks")):
            print(json.dumps(bench_rate(S, t, a, dev)), flush=True)
        return
    if a.live_video:
        for S, t in zip(a.streams, per_count(a.ticks, len(a.streams), "ticks")):
            print(json.dumps(bench_live(S, t, a, dev)), flush=True)
        return
    ticks = per_count(a.ticks, len(a.streams), "ticks")
    paced = per_count(a.paced_ticks, len(a.streams), "paced_ticks")
    for S, t, pt in zip(a.streams, ticks, paced):
        print(json.dumps(bench_one(S, t, pt, a, dev)), flush=True)


if __name__ == "__main__":
    main()
