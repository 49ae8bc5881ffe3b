"""The opt-in bf16-storage S3FD detector (`precision="bf16"`, `--face_det_precision bf16`): its glue kernels, the fused detection
head, every backbone geometry on the convb launches, the whole detector against the fp64 oracle within the bf16 error model's
yardstick, rects, determinism, weight invalidation, the 2 GiB size rule and the command line.

Yardstick: oracle.error_models.bf16_storage_noise jitters every conv input, weight and output of oracle/s3fd_ref.py (in fp64) by
the bf16 rounding bound; the largest move it causes over three seeds, per level, for scores and for box coordinates separately,
is what bf16 storage alone can do.  The HIP tables may be at most twice that far from the clean oracle (L-inf and mean)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import error_models, s3fd_ref
from wav2lip_amd import _lib, bf16
from wav2lip_amd import synthetic as synth
from wav2lip_amd._lib import ACT_RELU, check, ptr

pytestmark = pytest.mark.gpu

LEVELS = [(256, 4), (512, 2), (512, 2), (1024, 2), (512, 2), (256, 2)]      # (cin, ncls) of the six heads, net_s3fd.py:50-66


def _detector(cuda, seed=0, precision="bf16"):
    from wav2lip_amd import face_detection as fd
    return fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=synth.s3fd_state_dict(seed), precision=precision)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


# ---------------------------------------------------------------- glue kernels
def test_pack_bf16_equals_the_fp32_pack_with_zero_pad_channels(cuda):
    lib, s = _lib.load(), _lib.current_stream()
    img = np.random.default_rng(0).integers(0, 256, (2, 9, 7, 3), dtype=np.uint8)
    img[0, 0, 0], img[0, 0, 1] = 0, 255                     # the extremes: |v| <= 152
    g = torch.from_numpy(img).to(cuda)
    f32 = torch.zeros(2, 9, 7, 4, device=cuda)
    check(lib.w2l_s3fd_pack(s, 2 * 9 * 7, ptr(g), ptr(f32), 4))
    for cs in (8, 24):
        out = torch.full((2, 9, 7, cs), 5.0, device=cuda, dtype=torch.bfloat16)
        check(lib.w2l_s3fd_pack_bf16(s, 2 * 9 * 7, ptr(g), ptr(out), cs))
        assert torch.equal(out[..., :3].float().cpu(), f32[..., :3].cpu())
        assert bool((out[..., 3:] == 0).all())


@pytest.mark.parametrize("N,H,W,C,cs", [(2, 11, 14, 64, 64), (1, 7, 9, 24, 40), (3, 2, 3, 8, 8), (1, 5, 5, 512, 512)])
def test_maxpool_bf16_is_bit_equal_to_torch(cuda, N, H, W, C, cs):
    lib, s = _lib.load(), _lib.current_stream()
    g = torch.Generator().manual_seed(N * H + W)
    x = (torch.randn(N, H, W, cs, generator=g) * 10).to(torch.bfloat16)
    xg = x.to(cuda)
    y = torch.full((N, H // 2, W // 2, cs), 3.0, device=cuda, dtype=torch.bfloat16)
    check(lib.w2l_maxpool2x2_bf16(s, N, H, W, C, ptr(xg), cs, ptr(y), cs))
    ref = F.max_pool2d(x[..., :C].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(_bits(y[..., :C]), _bits(ref))
    assert bool((y[..., C:] == 3.0).all())                  # channels past C are not written


@pytest.mark.parametrize("C,x_cs", [(256, 256), (512, 520), (1024, 1024), (24, 32)])
def test_l2norm_bf16_within_one_rounding_of_fp64(cuda, C, x_cs):
    lib, s = _lib.load(), _lib.current_stream()
    g = torch.Generator().manual_seed(C)
    x = (torch.relu(torch.randn(2, 5, 7, x_cs, generator=g)) * 4).to(torch.bfloat16)
    w = torch.rand(C, generator=g) * 10
    xg, wg = x.to(cuda), w.to(cuda)
    y = torch.zeros(2, 5, 7, x_cs, device=cuda, dtype=torch.bfloat16)
    check(lib.w2l_l2norm_scale_bf16(s, 2 * 5 * 7, C, ptr(xg), x_cs, ptr(wg), ptr(y), x_cs))
    x64 = x[..., :C].double()
    ref = x64 / (x64.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10) * w.double()
    err = (y[..., :C].cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() * (1 + 1e-4) + 1e-30).all()), float((err / ref.abs().clamp_min(1e-30)).max())


# ---------------------------------------------------------------- fused head
def _fp32_decode(conf, loc, ncls, stride):
    """the existing path: fp32 NHWC conf / loc maps through w2l_s3fd_decode"""
    B, FH, FW = conf.shape[:3]
    out = torch.empty((B, FH * FW, 5), device=conf.device)
    check(_lib.load().w2l_s3fd_decode(_lib.current_stream(), B, FH, FW, stride, ptr(conf), ncls, ncls, ptr(loc), 4, ptr(out)))
    return out


@pytest.mark.parametrize("level,B,FH,FW,extra", [(0, 2, 13, 21, 0), (1, 1, 9, 17, 16), (2, 2, 5, 7, 0), (3, 1, 7, 3, 8),
                                                 (4, 2, 3, 1, 0), (5, 3, 1, 1, 24)])
def test_fused_head_against_fp64_conv_and_the_fp32_decode(cuda, level, B, FH, FW, extra):
    from wav2lip_amd.face_detection.s3fd import _HeadB
    cin, ncls = LEVELS[level]
    stride = 2 ** (level + 2)
    g = torch.Generator().manual_seed(level)
    x_cs = cin + extra
    x = (torch.relu(torch.randn(B, FH, FW, x_cs, generator=g)) * 2).to(torch.bfloat16)
    conf = torch.nn.Conv2d(cin, ncls, 3, padding=1)
    loc = torch.nn.Conv2d(cin, 4, 3, padding=1)
    with torch.no_grad():
        for m in (conf, loc):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (cin * 9)) ** 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
    conf, loc = conf.to(cuda), loc.to(cuda)
    head = _HeadB(conf, loc, ncls)
    out = torch.full((B, FH * FW, 5), float("nan"), device=cuda)
    xb = bf16.ActB(x.to(cuda), 0, cin)
    head.decode(xb, stride, out)
    x64 = x[..., :cin].permute(0, 3, 1, 2).double()
    maps = []
    for m in (conf, loc):
        w64 = m.weight.detach().cpu().to(torch.bfloat16).double()
        y = F.conv2d(x64, w64, m.bias.detach().cpu().double(), padding=1)
        maps.append(y.float().permute(0, 2, 3, 1).contiguous().to(cuda))
    ref = _fp32_decode(maps[0], maps[1], ncls, stride).cpu()
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    assert float((got[..., 4] - ref[..., 4]).abs().max()) <= 1e-5
    assert float((got[..., :4] - ref[..., :4]).abs().max()) <= 1e-4 * stride * 4


# ---------------------------------------------------------------- backbone geometries on convb
def _backbone_layers():
    from wav2lip_amd.face_detection.s3fd import BACKBONE
    return [it for it in BACKBONE if not isinstance(it, str)]


@pytest.mark.parametrize("name,cin,cout,k,st,p", _backbone_layers(), ids=lambda v: str(v))
def test_every_backbone_geometry_on_convb_against_fp64(cuda, name, cin, cout, k, st, p):
    _convb_check(cuda, cin, cout, k, st, p, N=2, H=13, W=10, seed=cin + cout)


def test_conv1_2_at_480x640_large_m(cuda):
    _convb_check(cuda, 64, 64, 3, 1, 1, N=1, H=480, W=640, seed=7, family="igemm")       # 1200 tiles: under the box kernel's rule


def test_conv1_2_at_480x640_on_the_resident_box_kernel(cuda):
    """two frames: 2400 16x16 tiles, over the 2048-tile rule - conv1_2 of the benchmarked detector batches runs on box64"""
    _convb_check(cuda, 64, 64, 3, 1, 1, N=2, H=480, W=640, seed=8, family="box64")


def _convb_check(cuda, cin, cout, k, st, p, N, H, W, seed, family=None):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, stride=st, padding=p)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    conv = conv.to(cuda)
    f = bf16.FoldedConvB(conv, None, ACT_RELU)
    x = torch.zeros(N, H, W, bf16.round8(cin), dtype=torch.bfloat16)
    x[..., :cin] = torch.randn(N, H, W, cin, generator=g).to(torch.bfloat16)
    ho, wo = f.layer.out_hw(H, W)
    y = bf16.new_buf(N, ho, wo, cout, cuda)
    f.layer.run(bf16.ActB(x.to(cuda), 0, cin), bf16.ActB(y, 0, cout), scale=f.scale, shift=f.shift)
    w64 = conv.weight.detach().cpu().to(torch.bfloat16).double()
    ref = torch.relu(F.conv2d(x[..., :cin].permute(0, 3, 1, 2).double(), w64, conv.bias.detach().cpu().double(), stride=st, padding=p))
    got = y.cpu().double().permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    tol = 2.0 ** -8 * ref.abs() + 1e-5 * float(ref.abs().max())
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float((got - ref).abs().max()))
    if family is not None:
        assert f.layer.resolve(N, H, W)[0] == family


# ---------------------------------------------------------------- whole detector against the oracle
def _frame_sets():
    """the golden frames, three more seeds of them and one larger frame"""
    return [synth.s3fd_frames(seed=k) for k in (1, 2, 3, 4)] + [synth.s3fd_frames(B=1, H=192, W=256)]


def _geometry_sets():
    """production-like and edge geometries: 480x640 (conv1_2 over the box kernel's 2048-tile rule at B = 2, as in the benchmarked
    B = 16 batches), 250x333 (extents no power of two divides: odd pooled maps, ragged head boxes, fc6's padding of 3 on an odd
    map) and 33x47, the smallest kind of frame the network takes (pool5 is 1x1; fc6's padding makes fc7 5x5, so no level is
    narrower than 2)"""
    return [synth.s3fd_frames(seed=6, B=2, H=480, W=640), synth.s3fd_frames(seed=7, B=3, H=250, W=333),
            synth.s3fd_frames(seed=8, B=2, H=33, W=47)]


def _oracle_runs(frame_sets):
    """per frame set: the clean fp64 oracle's dense tables and those of three bf16_storage_noise seeds"""
    torch.set_num_threads(16)
    sd64 = {k: v.double() for k, v in synth.s3fd_state_dict(0).items()}
    runs = []
    with torch.no_grad():
        for img in frame_sets:
            x = s3fd_ref.preprocess(img).double()
            clean = s3fd_ref.dense_boxes(s3fd_ref.s3fd_forward(sd64, x))
            noisy = []
            for seed in range(3):
                with error_models.bf16_storage_noise(seed):
                    noisy.append(s3fd_ref.dense_boxes(s3fd_ref.s3fd_forward(sd64, x)))
            runs.append((img, clean, noisy))
    return runs


@pytest.fixture(scope="module")
def oracle_runs():
    return _oracle_runs(_frame_sets())


@pytest.fixture(scope="module")
def geometry_runs():
    return _oracle_runs(_geometry_sets())


def test_whole_detector_against_the_oracle_within_the_yardstick(cuda, oracle_runs):
    _dense_within_the_yardstick(cuda, oracle_runs)


def test_whole_detector_at_production_and_edge_geometries(cuda, geometry_runs):
    """the yardstick at the geometries of _geometry_sets; at 480x640 the plan must run conv1_2 on box64"""
    fa = _detector(cuda)
    _dense_within_the_yardstick(cuda, geometry_runs, fa)
    for img, _, _ in geometry_runs:
        B, H, W = img.shape[:3]
        disp = fa.face_detector._graph(B, H, W, torch.device(cuda), precision="bf16").dispatch()
        print("%dx%dx%d: %s" % (B, H, W, ", ".join("%s %s%s" % (n, f, "" if f != "igemm" else " t%d k%d" % (t, k))
                                                    for n, f, t, k in disp)))
        assert len(disp) == len(_backbone_layers())
        if (H, W) == (480, 640):
            assert dict((n, f) for n, f, _, _ in disp)["conv1_2"] == "box64", disp


def test_fp32_detector_against_the_oracle(cuda, oracle_runs, geometry_runs):
    """the fp32 detector's dense tables against the same clean fp64 oracle, at the tolerance of test_s3fd_gpu.py"""
    fa = _detector(cuda, precision="f32")
    for img, clean, _ in oracle_runs + geometry_runs:
        got = [t.cpu().double().numpy() for t in fa.face_detector.dense_boxes(torch.from_numpy(img).to(cuda))]
        assert len(got) == len(clean) == 6
        for lv, (g, c) in enumerate(zip(got, clean)):
            assert g.shape == c.shape
            err = float(np.abs(g - c).max())
            print("fp32 %s level %d: L-inf %.3e" % (img.shape, lv, err))
            assert err <= 2e-3, (img.shape, lv, err)


def _dense_within_the_yardstick(cuda, runs, fa=None):
    fa = fa or _detector(cuda)
    for img, clean, noisy in runs:
        got = [t.cpu().double().numpy() for t in fa.face_detector.dense_boxes(torch.from_numpy(img).to(cuda), precision="bf16")]
        assert len(got) == len(clean) == 6
        for lv, (g, c) in enumerate(zip(got, clean)):
            assert g.shape == c.shape
            for part, sl in (("score", slice(4, 5)), ("coords", slice(0, 4))):
                yl = max(float(np.abs(n[lv][..., sl] - c[..., sl]).max()) for n in noisy)
                ym = max(float(np.abs(n[lv][..., sl] - c[..., sl]).mean()) for n in noisy)
                d = np.abs(g[..., sl] - c[..., sl])
                print("%s level %d %s: L-inf %.3e (yardstick %.3e), mean %.3e (%.3e)" % (img.shape, lv, part, d.max(), yl, d.mean(), ym))
                assert float(d.max()) <= 2 * yl, (img.shape, lv, part)
                assert float(d.mean()) <= 2 * ym, (img.shape, lv, part)


def test_rects_of_robust_coordinates_match_the_oracle(cuda, oracle_runs):
    assert _rects_match(cuda, oracle_runs) >= 1


def test_rects_at_production_and_edge_geometries(cuda, geometry_runs):
    assert _rects_match(cuda, geometry_runs) >= 1


def _rects_match(cuda, runs):
    """A rect coordinate is robust when every noisy oracle run gives the clean oracle's value; there the bf16 rect equals it within
    one pixel (truncation to int).  (Per coordinate, not per image: with the seeded weights bf16_storage_noise moves at least one
    coordinate of every test image by 1-2 pixels.)  Every other coordinate stays within twice the noisy runs' largest move plus
    one pixel, and an image where every oracle run finds a face gets one from bf16 as well."""
    fa = _detector(cuda)
    robust = 0
    for img, clean, noisy in runs:
        want = s3fd_ref.rects(s3fd_ref.detections(clean))
        alts = [s3fd_ref.rects(s3fd_ref.detections(n)) for n in noisy]
        got = fa.get_detections_for_batch(img)
        for b in range(len(img)):
            print("image %s/%d: oracle %s, noisy %s, bf16 %s" % (img.shape, b, want[b], [a[b] for a in alts], got[b]))
            if want[b] is None or any(a[b] is None for a in alts):
                continue
            assert got[b] is not None
            for k in range(4):
                move = max(abs(a[b][k] - want[b][k]) for a in alts)
                if move == 0:
                    robust += 1
                    assert abs(got[b][k] - want[b][k]) <= 1, (b, k, got[b], want[b])
                else:
                    assert abs(got[b][k] - want[b][k]) <= 2 * move + 1, (b, k, got[b], want[b], move)
    return robust


# ---------------------------------------------------------------- determinism, invalidation
def test_two_calls_are_bit_identical_and_new_weights_rebuild(cuda):
    img = torch.from_numpy(synth.s3fd_frames()).to(cuda)
    fa = _detector(cuda)
    net = fa.face_detector
    a = [t.clone() for t in net.dense_boxes(img, precision="bf16")]
    b = [t.clone() for t in net.dense_boxes(img, precision="bf16")]
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    net.load_state_dict(synth.s3fd_state_dict(1))
    c = [t.clone() for t in net.dense_boxes(img, precision="bf16")]
    assert not all(torch.equal(u, v) for u, v in zip(a, c))
    fresh = _detector(cuda, seed=1).face_detector.dense_boxes(img, precision="bf16")
    assert all(torch.equal(u, v) for u, v in zip(c, fresh))


def test_fp32_tables_are_unchanged_by_a_bf16_run(cuda):
    img = torch.from_numpy(synth.s3fd_frames()).to(cuda)
    net = _detector(cuda).face_detector
    a = [t.clone() for t in net.dense_boxes(img)]
    net.dense_boxes(img, precision="bf16")
    b = net.dense_boxes(img)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        net.dense_boxes(img, precision="fp16")


# ---------------------------------------------------------------- size rule
def test_a_batch_over_the_2gib_rule_raises_before_allocating(cuda):
    net = _detector(cuda).face_detector
    img = torch.zeros((16, 1088, 1920, 3), dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match="2 GiB"):
        net.dense_boxes(img, precision="bf16")
    assert torch.cuda.memory_allocated() == before


def test_face_detect_halves_the_batch_and_returns_the_direct_rects(cuda, capsys):
    """16 frames of 1080 x 1920: the batch of 16 is over the rule (conv1's activations: 4.2 GB), _detect_rects halves it; a batch
    of 8 is under it (2.12e9 bytes < 2**31), so the rects are those of a direct run in batches of 8"""
    from wav2lip_amd import inference
    fa = _detector(cuda)
    r = np.random.default_rng(4)
    frames = [r.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(16)]
    for f in frames:
        f[300:700, 800:1300] = 255
    rects = inference._detect_rects(frames, fa, 16)
    assert "New batch size: 8" in capsys.readouterr().out
    direct = []
    for lo in range(0, 16, 8):
        direct += fa.get_detections_for_batch(np.array(frames[lo:lo + 8]))
    assert rects == direct
    if all(d is not None for d in direct):
        # the same through face_detect with an fp32 detector asked for bf16 (pads 0, no smoothing: the boxes are the rects)
        crops = inference.face_detect(frames, _detector(cuda, precision="f32"), pads=(0, 0, 0, 0), nosmooth=True, batch_size=16,
                                      precision="bf16")
        want = [(max(0, x1), max(0, y1), min(1920, x2), min(1080, y2)) for x1, y1, x2, y2 in direct]    # face_detect's clipping
        assert [(x1, y1, x2, y2) for _, (y1, y2, x1, x2) in crops] == want


# ---------------------------------------------------------------- command line
def test_cli_face_det_precision_bf16_end_to_end(cuda, tmp_path, monkeypatch):
    from scipy.io import wavfile
    from wav2lip_amd import container, inference
    from wav2lip_amd import models as amd_models
    from wav2lip_amd.face_detection import api
    from wav2lip_amd.face_detection.s3fd import s3fd as S3FD
    tmp = str(tmp_path)
    torch.save(synth.s3fd_state_dict(0), f"{tmp}/s3fd.pth")
    monkeypatch.setattr(api, "DEFAULT_WEIGHTS", f"{tmp}/s3fd.pth")
    seen = []
    real = S3FD.dense_boxes

    def spy(self, images, precision="f32"):
        seen.append(precision)
        return real(self, images, precision=precision)

    monkeypatch.setattr(S3FD, "dense_boxes", spy)
    img = synth.s3fd_frames()
    w = container.AviWriter(f"{tmp}/clip.avi", 25.0, (img.shape[2], img.shape[1]))
    w.__enter__()
    for k in range(4):
        w.write(img[k % 2])
    w.__exit__(None, None, None)
    wav = synth.sine_wav(1.0)
    wavfile.write(f"{tmp}/audio.wav", 16000, np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16))
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in amd_models.Wav2Lip().state_dict().items()}, seed=0)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer": None, "global_step": 7, "global_epoch": 1},
               f"{tmp}/ckpt.pth")
    monkeypatch.setattr(inference, "args", inference.args)        # main() replaces the module-level args
    frames = inference.main(["--checkpoint_path", f"{tmp}/ckpt.pth", "--face", f"{tmp}/clip.avi", "--audio", f"{tmp}/audio.wav",
                             "--outfile", f"{tmp}/out.avi", "--face_det_precision", "bf16", "--wav2lip_batch_size", "16"])
    assert inference.args.face_det_precision == "bf16" and inference.args.precision == "fp32"
    assert seen and set(seen) == {"bf16"}
    assert len(frames) >= 4 and frames[0].shape == img.shape[1:]
    clip = container.read_avi(f"{tmp}/out.avi")
    assert len(clip["frames"]) == len(frames)
