"""The opt-in bf16-storage inference path (`precision="bf16"`): input kernels, the fused output block, whole batches against the
CPU oracle within the bf16 error model's yardstick, stability, determinism and the command line.

Yardstick: oracle.error_models.bf16_storage_noise jitters every conv input, weight and output of the exact graph by the bf16
rounding bound; the largest move it causes over three seeds (first 16 frames of BASELINE cfg2) is what bf16 storage alone can
do.  The HIP path may be at most twice that far from the oracle (L-inf and mean), and its uint8 frames at most one level worse."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import datagen_ref, error_models, models_ref
from wav2lip_amd import synthetic as synth
from wav2lip_amd import models as amd_models

pytestmark = pytest.mark.gpu


def _load(seed, cuda):
    G = amd_models.Wav2Lip()
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=seed)
    G.load_state_dict(sd)
    return G.to(cuda).eval(), sd


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _u8(x):
    return datagen_ref.frames_to_u8(np.asarray(x, dtype=np.float32))


@pytest.fixture(scope="module")
def yardstick():
    """max over seeds 0-2 of the move bf16_storage_noise causes on the first 16 frames of BASELINE cfg2"""
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in amd_models.Wav2Lip().state_dict().items()}, seed=0)
    img, mel = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(synth.face_crops_u8(16, seed=5), synth.mel_windows(16, seed=5)))
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    m64, i64 = torch.from_numpy(mel).double(), torch.from_numpy(img).double()
    with torch.no_grad():
        clean = models_ref.wav2lip_forward(sd64, m64, i64)
        linf, mean, worst = 0.0, 0.0, 0
        for seed in range(3):
            with error_models.bf16_storage_noise(seed):
                noisy = models_ref.wav2lip_forward(sd64, m64, i64)
            d = (noisy - clean).abs()
            linf, mean = max(linf, float(d.max())), max(mean, float(d.mean()))
            du = np.abs(_u8(noisy.numpy()).astype(np.int32) - _u8(clean.numpy()).astype(np.int32))
            worst = max(worst, int(du.max()))
    y = {"linf": linf, "mean": mean, "u8": worst}
    print("bf16 yardstick (max over 3 seeds, 16 frames): L-inf %.3e, mean %.3e, worst uint8 level %d" % (linf, mean, worst))
    return y


# ---------------------------------------------------------------- input kernels
def test_datagen_pack_bf16_is_the_rounded_fp32_packing(cuda):
    from wav2lip_amd import _lib
    lib = _lib.load()
    for n in (1, 7):
        faces = synth.face_crops_u8(n, seed=3 + n)
        img, _ = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(faces, synth.mel_windows(n, seed=1)))
        ref = torch.zeros((n, 96, 96, 8), dtype=torch.float32)
        ref[..., :6] = torch.from_numpy(img).permute(0, 2, 3, 1)
        y = torch.full((n, 96, 96, 8), 7.0, dtype=torch.bfloat16, device=cuda)        # pad channels must be written
        f = torch.from_numpy(faces).to(cuda)
        _lib.check(lib.w2l_datagen_pack_bf16(_lib.current_stream(), n, 96, _lib.ptr(f), _lib.ptr(y), 8, 8), "datagen_pack_bf16")
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(ref.to(torch.bfloat16))), n


def test_mel_gather_bf16_is_the_rounded_fp32_gather_with_ragged_starts(cuda):
    from wav2lip_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(11)
    T = 203
    mel = rng.uniform(-4, 4, (80, T)).astype(np.float32)
    starts = np.array([0, 3, 3, 187, 50, 1, 120, 99, 186, 17, 160], dtype=np.int32)    # ragged: uneven, repeated, out of order
    B = len(starts)
    ref = torch.zeros((B, 80, 16, 8), dtype=torch.float32)
    for b, s in enumerate(starts):
        ref[b, :, :, 0] = torch.from_numpy(mel[:, s:s + 16])
    out = torch.full((B, 80, 16, 8), 5.0, dtype=torch.bfloat16, device=cuda)
    m, st = torch.from_numpy(mel).to(cuda), torch.from_numpy(starts).to(cuda)
    _lib.check(lib.w2l_mel_gather_bf16(_lib.current_stream(), _lib.ptr(m), T, _lib.ptr(st), B, _lib.ptr(out), 8, 8), "mel_gather_bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref.to(torch.bfloat16)))


# ---------------------------------------------------------------- output block
@pytest.mark.parametrize("N", [1, 7, 128])
def test_output_block_bf16_against_fp64(cuda, N):
    from wav2lip_amd import bf16, engine
    from wav2lip_amd._lib import ACT_RELU, ACT_SIGMOID, ConvGeom
    gen = torch.Generator().manual_seed(N)
    w = torch.randn(32, 80, 3, 3, generator=gen) * 0.05
    hconv = torch.nn.Conv2d(32, 3, 1)
    with torch.no_grad():
        hconv.weight.copy_(torch.randn(3, 32, 1, 1, generator=gen) * 0.3)
        hconv.bias.copy_(torch.randn(3, generator=gen) * 0.1)
    scale = torch.rand(32, generator=gen) + 0.5
    shift = torch.randn(32, generator=gen) * 0.1
    x = (torch.rand(N, 96, 96, 80, generator=gen) * 2).to(torch.bfloat16)
    layer = bf16.ConvB(ConvGeom(0, 80, 32, 3, 3, 1, 1, 1, 1, 0, 0, ACT_RELU), w.to(cuda))
    layer.attach_head(w.to(cuda), hconv.to(cuda), ACT_SIGMOID)
    xd = x.to(cuda)
    frames = torch.empty((N, 96, 96, 3), dtype=torch.uint8, device=cuda)
    out32 = engine.Act(engine.new_buf(N, 96, 96, 4, cuda, zero=True), 0, 3)
    layer.forward_head(bf16.ActB(xd, 0, 80), frames, out32, scale.to(cuda), shift.to(cuda))
    torch.cuda.synchronize()
    got = out32.buf[..., :3].cpu()
    # fp64 over the same bf16-rounded input and weights; scale / shift / head in fp64 from their fp32 values
    xr = x.double().permute(0, 3, 1, 2)
    wr = w.to(torch.bfloat16).double()
    z = torch.nn.functional.conv2d(xr, wr, padding=1)
    a = torch.relu(z * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    ref = torch.sigmoid(torch.nn.functional.conv2d(a, hconv.weight.detach().cpu().double(), hconv.bias.detach().cpu().double()))
    ref = ref.permute(0, 2, 3, 1)
    # fp32 accumulation of 720 products of magnitude <= |x||w|: a few ulp of sum|x w| before the (<= 0.25-slope) sigmoid
    bound = 1e-6 * float((torch.nn.functional.conv2d(xr.abs(), wr.abs(), padding=1).max())) + 1e-6
    err = float((got.double() - ref).abs().max())
    print("N=%d output block L-inf vs fp64 %.3e (bound %.3e)" % (N, err, bound))
    assert err <= bound, (err, bound)
    own = (got.numpy() * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(frames.cpu().numpy(), own)


# ---------------------------------------------------------------- whole batches
def _run_bf16(G, faces, mels, cuda, runner=None):
    from wav2lip_amd.inference import Wav2LipRunner
    r = runner or Wav2LipRunner(G, batch_size=len(faces), precision="bf16")
    u8 = r.run_batch(torch.from_numpy(faces).to(cuda), torch.from_numpy(mels).to(cuda)).cpu().numpy().copy()
    return u8, r.last_pred_nchw().cpu()


@pytest.fixture(scope="module")
def cfg2_oracle():
    """the 128 BASELINE cfg2 frames (face_crops_u8 / mel_windows, seed 5) and the CPU oracle's prediction for them under the seed-0
    weights: (faces, mels, prediction [128,3,96,96])"""
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in amd_models.Wav2Lip().state_dict().items()}, seed=0)
    faces, mels = synth.face_crops_u8(128, seed=5), synth.mel_windows(128, seed=5)
    img, mel = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(faces, mels))
    with torch.no_grad():
        ref = torch.cat([models_ref.wav2lip_forward(sd, torch.from_numpy(mel[lo:lo + 16]), torch.from_numpy(img[lo:lo + 16]))
                         for lo in range(0, 128, 16)])
    return faces, mels, ref


def _against_the_oracle(label, u8, y, ref, ref_u8, yardstick):
    """the yardstick assertions: prediction `y` (or None) within twice the yardstick of `ref` (L-inf and mean), the uint8 frames
    `u8` the truncation of `y` and at most one level further from the oracle's frames `ref_u8` than the yardstick allows"""
    du = np.abs(u8.astype(np.int32) - ref_u8.astype(np.int32))
    msg = "bf16 vs oracle, %s: uint8: %.2f %% of bytes differ, worst %d levels (yardstick %d)" % (
        label, 100.0 * float((du != 0).mean()), int(du.max()), yardstick["u8"])
    if y is not None:
        d = (y - ref).abs()
        linf, mean = float(d.max()), float(d.mean())
        msg += "; L-inf %.3e (yardstick %.3e), mean %.3e (yardstick %.3e)" % (linf, yardstick["linf"], mean, yardstick["mean"])
        assert np.array_equal(u8, _u8(y.numpy())), msg               # the frames are the truncation of the fp32 prediction
    print(msg)
    if y is not None:
        assert linf <= 2 * yardstick["linf"], msg
        assert mean <= 2 * yardstick["mean"], msg
    assert int(du.max()) <= yardstick["u8"] + 1, msg


def test_baseline_cfg2_batch_against_the_oracle_within_the_yardstick(cuda, yardstick, cfg2_oracle):
    G, _ = _load(0, cuda)
    faces, mels, ref = cfg2_oracle
    u8, y = _run_bf16(G, faces, mels, cuda)
    _against_the_oracle("128 frames", u8, y, ref, _u8(ref.numpy()), yardstick)


def _dispatch_map(G):
    """{N: ((record, family, tile, ksplit), ...)} of the bf16 generator plan for N = 1..MAX_PLAN_BATCH (ConvB.resolve: the launcher's
    own rules, nothing launched)"""
    from wav2lip_amd.inference import Wav2LipRunner
    g = Wav2LipRunner(G, batch_size=1, precision="bf16")._graph(1)
    return {n: tuple(g.dispatch(n)) for n in range(1, G.MAX_PLAN_BATCH + 1)}


def _chunks(n, cap):
    return [min(cap, n - lo) for lo in range(0, n, cap)]


def _pick_batch_sizes(dmap, fixed, cap):
    """`fixed` plus a greedy cover of every (record, family) pair and every (record, tile, split-K) an igemm launch takes in `dmap`"""
    def keys(n):
        out = set()
        for name, fam, tile, ks in dmap[n]:
            out.add((name, fam))
            if fam == "igemm":
                out.add((name, fam, tile, ks))
        return out
    want = set().union(*(keys(n) for n in dmap))
    sizes = set(fixed)
    have = set().union(*(keys(c) for n in sizes for c in _chunks(n, cap)))
    while want - have:
        best = max(sorted(dmap), key=lambda n: len(keys(n) - have))      # ties: the smallest batch
        sizes.add(best)
        have |= keys(best)
    return sorted(sizes), want


def _boundaries(dmap):
    """per record: [(first N, family, tile, ksplit)] at every N where its launch changes"""
    out = {}
    for n in sorted(dmap):
        for name, fam, tile, ks in dmap[n]:
            seq = out.setdefault(name, [])
            if not seq or seq[-1][1:] != (fam, tile, ks):
                seq.append((n, fam, tile, ks))
    return out


def test_bf16_batch_sizes_across_the_dispatch_map_against_the_oracle(cuda, yardstick, cfg2_oracle):
    """The same layer runs a different kernel (stem / box64 / tp2b / igemm with its tile and split-K) at different batch sizes.
    Batch sizes chosen from the dispatch map so that every (layer, family) and every (layer, igemm tile, split-K) the plans take
    runs once, plus 1, 2, 128, 129, 512 and a chunked 600 (512 + 88): input j is pool frame j mod 128, so one oracle run serves
    every size.  Each size is held to the yardstick; frames with identical inputs are bit-identical within a batch (folded
    BatchNorm: no result depends on a frame's position in M - tile masking and the split-K workspace are what would break it),
    and two sizes whose launches all resolve alike agree bit for bit on the frames they share."""
    from wav2lip_amd.inference import Wav2LipRunner
    G, _ = _load(0, cuda)
    cap = G.MAX_PLAN_BATCH
    dmap = _dispatch_map(G)
    sizes, want = _pick_batch_sizes(dmap, (1, 2, 128, 129, 512, 600), cap)
    for n0 in (15, 129):                   # and the largest batch that resolves every launch as n0 does: more M tiles, same kernels
        sizes = sorted(set(sizes) | {n0, max(n for n in dmap if dmap[n] == dmap[n0])})
    bounds = _boundaries(dmap)
    for name, seq in bounds.items():
        print("%-28s %s" % (name, "  ".join("N>=%d: %s%s" % (n, f, "" if f != "igemm" else " t%d k%d" % (t, k)) for n, f, t, k in seq)))
    print("batch sizes: %s (%d (layer, family / tile, split-K) keys)" % (sizes, len(want)))
    fams = {fam for m in dmap.values() for _, fam, _, _ in m}
    assert {"igemm", "box64", "tp2b", "k3s_head"} <= fams and any(f.startswith("stem") for f in fams), fams
    faces, mels, ref = cfg2_oracle
    ref_u8 = _u8(ref.numpy())
    sig_count = {}
    for n in sizes:
        if n <= cap:
            sig_count[dmap[n]] = sig_count.get(dmap[n], 0) + 1
    shared, compared = {}, 0
    for n in sizes:
        G._graphs.clear()                  # one resident plan at a time
        idx = np.arange(n) % 128
        r = Wav2LipRunner(G, batch_size=n, precision="bf16")
        u8, y = _run_bf16(G, faces[idx], mels[idx], cuda, r)
        del r
        last = _chunks(n, cap)[-1]
        lo = n - last                      # last_pred_nchw covers the last chunk
        if lo:
            _against_the_oracle("N=%d (first %d frames)" % (n, lo), u8[:lo], None, None, ref_u8[idx[:lo]], yardstick)
        _against_the_oracle("N=%d%s" % (n, "" if not lo else " (last chunk of %d)" % last), u8[lo:], y, ref[idx[lo:]],
                            ref_u8[idx[lo:]], yardstick)
        pos = np.arange(n)
        dup = pos[pos - 128 >= pos // cap * cap]     # frame j and frame j - 128 of the same chunk (plan) have identical inputs
        assert np.array_equal(u8[dup], u8[dup - 128]), "N=%d: frames with identical inputs differ" % n
        if lo == 0 and len(dup):
            yb = _bits(y)
            assert torch.equal(yb[dup], yb[dup - 128]), "N=%d: predictions with identical inputs differ" % n
        if n <= cap and sig_count[dmap[n]] > 1:
            prev = shared.get(dmap[n])
            if prev is None:
                shared[dmap[n]] = (n, _bits(y[:128]), u8[:128].copy())
            else:
                m = min(n, prev[0], 128)
                assert torch.equal(_bits(y[:m]), prev[1][:m]) and np.array_equal(u8[:m], prev[2][:m]), \
                    "N=%d and N=%d resolve alike but differ" % (prev[0], n)
                compared += 1
    G._graphs.clear()
    print("%d batch sizes compared bit for bit with another size of the same dispatch" % compared)
    assert compared >= 2


def test_same_batch_twice_gives_identical_bytes(cuda):
    G, _ = _load(0, cuda)
    faces, mels = synth.face_crops_u8(16, seed=2), synth.mel_windows(16, seed=2)
    from wav2lip_amd.inference import Wav2LipRunner
    r = Wav2LipRunner(G, batch_size=16, precision="bf16")
    a, _ = _run_bf16(G, faces, mels, cuda, r)
    b, _ = _run_bf16(G, faces, mels, cuda, r)
    assert np.array_equal(a, b)


def test_pipelined_runner_matches_the_plain_runner(cuda):
    from wav2lip_amd.inference import PipelinedRunner
    G, _ = _load(0, cuda)
    batches = [(synth.face_crops_u8(32, seed=20 + i), synth.mel_windows(32, seed=20 + i)) for i in range(6)]
    ref = [_run_bf16(G, f, m, cuda)[0] for f, m in batches]
    pr = PipelinedRunner(G, 32, depth=4, precision="bf16")
    tickets = [pr.submit(torch.from_numpy(f).to(cuda), torch.from_numpy(m).to(cuda)) for f, m in batches[:4]]
    got = []
    for i, (f, m) in enumerate(batches[4:]):
        got.append(pr.result(tickets[i]).cpu().numpy().copy())
        tickets.append(pr.submit(torch.from_numpy(f).to(cuda), torch.from_numpy(m).to(cuda)))
    for t in tickets[2:]:
        got.append(pr.result(t).cpu().numpy().copy())
    for i, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), i


def test_run_frames_equals_run_batch_plus_paste(cuda):
    from wav2lip_amd import _lib
    from wav2lip_amd.inference import Wav2LipRunner
    lib = _lib.load()
    G, _ = _load(0, cuda)
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (3, 160, 200, 3), dtype=np.uint8)).to(cuda)
    boxes = [(10, 130, 20, 140), (0, 96, 0, 96), (30, 150, 50, 200), (5, 105, 60, 170)]
    idx = [0, 1, 2, 1]
    mels = torch.from_numpy(synth.mel_windows(4, seed=9)).to(cuda)
    r = Wav2LipRunner(G, batch_size=4, precision="bf16")
    got = r.run_frames(frames, idx, boxes, mel_windows=mels).cpu().numpy()
    s = _lib.current_stream()
    bdev = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    idev = torch.tensor(idx, dtype=torch.int32, device=cuda)
    faces = torch.empty((4, 96, 96, 3), dtype=torch.uint8, device=cuda)
    _lib.check(lib.w2l_crop_resize_u8(s, 4, _lib.ptr(frames), 160, 200, _lib.ptr(idev), _lib.ptr(bdev), 96, _lib.ptr(faces)), "crop")
    pred = r.run_batch(faces, mel_windows=mels).clone()
    out = frames.index_select(0, idev.long())
    max_px = max((y2 - y1) * (x2 - x1) for y1, y2, x1, x2 in boxes)
    _lib.check(lib.w2l_resize_paste_u8(s, 4, _lib.ptr(pred), 96, _lib.ptr(bdev), None, _lib.ptr(out), 160, 200, max_px), "paste")
    assert np.array_equal(got, out.cpu().numpy())


def test_load_state_dict_rebuilds_the_plan(cuda):
    G, _ = _load(0, cuda)
    G1, sd1 = _load(1, cuda)
    faces, mels = synth.face_crops_u8(8, seed=4), synth.mel_windows(8, seed=4)
    from wav2lip_amd.inference import Wav2LipRunner
    r = Wav2LipRunner(G, batch_size=8, precision="bf16")
    a, _ = _run_bf16(G, faces, mels, cuda, r)
    G.load_state_dict({k: v.to(cuda) for k, v in sd1.items()})
    b, _ = _run_bf16(G, faces, mels, cuda, r)
    c, _ = _run_bf16(G1, faces, mels, cuda)
    assert not np.array_equal(a, b)
    assert np.array_equal(b, c)


def test_bad_precision_is_rejected(cuda):
    from wav2lip_amd.inference import PipelinedRunner, Wav2LipRunner, lipsync
    G, _ = _load(0, cuda)
    for bad in ("fp16", "fp32", None):
        with pytest.raises(ValueError):
            Wav2LipRunner(G, precision=bad)
        with pytest.raises(ValueError):
            PipelinedRunner(G, precision=bad)
        with pytest.raises(ValueError):
            lipsync(G, [np.zeros((96, 96, 3), np.uint8)], synth.sine_wav(1.0), precision=bad)
        with pytest.raises(ValueError):
            G.graph(4, precision=bad)


# ---------------------------------------------------------------- determinism across processes
_CHILD = r'''
import hashlib, sys
import torch
sys.path.insert(0, %r)
from wav2lip_amd import models
from wav2lip_amd import synthetic as synth
from wav2lip_amd.inference import Wav2LipRunner
dev = torch.device("cuda", 0)
G = models.Wav2Lip()
G.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0))
G = G.to(dev).eval()
r = Wav2LipRunner(G, batch_size=24, precision="bf16")
u8 = r.run_batch(torch.from_numpy(synth.face_crops_u8(24, seed=7)).to(dev), torch.from_numpy(synth.mel_windows(24, seed=7)).to(dev))
print("DIGEST " + hashlib.sha256(u8.cpu().numpy().tobytes()).hexdigest())
''' % ROOT


def _run_child():
    env = dict(os.environ)
    env.pop("W2L_AUTOTUNE", None)
    p = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return [l for l in p.stdout.splitlines() if l.startswith("DIGEST ")][-1]


def test_two_fresh_processes_produce_identical_bf16_frames():
    assert _run_child() == _run_child()


# ---------------------------------------------------------------- command line
def test_cli_precision_bf16_on_the_datapath_fixture(cuda, tmp_path, yardstick):
    from scipy.io import wavfile
    from PIL import Image
    from wav2lip_amd import inference
    G = np.load(os.path.join(ROOT, "tests", "golden", "golden_datapath_v1.npz"))
    tmp = str(tmp_path)
    Image.fromarray(np.ascontiguousarray(G["inf_face"][:, :, ::-1])).save(os.path.join(tmp, "face.png"))
    wav = synth.sine_wav(3.0)
    wavfile.write(os.path.join(tmp, "audio.wav"), 16000, np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16))
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in amd_models.Wav2Lip().state_dict().items()}, seed=0)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer": None, "global_step": 7, "global_epoch": 1},
               os.path.join(tmp, "ckpt.pth"))
    common = ["--checkpoint_path", os.path.join(tmp, "ckpt.pth"), "--face", os.path.join(tmp, "face.png"),
              "--audio", os.path.join(tmp, "audio.wav"), "--box", "0", "96", "0", "96", "--wav2lip_batch_size", "32"]
    f32 = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "a.avi")]))
    b16 = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "b.avi"), "--precision", "bf16"]))
    assert inference.args.precision == "bf16"
    assert b16.shape == f32.shape == (72, 96, 96, 3)
    d = np.abs(b16.astype(np.int32) - f32.astype(np.int32))
    print("CLI bf16 vs fp32: %.2f %% of bytes differ, worst %d levels, mean %.3e" % (100.0 * float((d != 0).mean()), int(d.max()),
                                                                                  float(d.mean()) / 255.0))
    assert int(d.max()) <= yardstick["u8"] + 1
    assert float(d.mean()) / 255.0 <= 2 * yardstick["mean"]
