"""Whole networks on the HIP path against (a) the committed outputs of the real reference and (b) the oracle,
north_star tolerance: 1e-3 L-inf on fp32 pixels (we assert 1e-4, the observed error is ~1e-6)."""
import numpy as np
import pytest
import torch

from oracle import datagen_ref, models_ref
from wav2lip_amd import synthetic as synth
from wav2lip_amd import models as amd_models

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _load(model, seed, cuda):
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed)
    model.load_state_dict(sd)
    return model.to(cuda).eval(), sd


def _gen_inputs(n, seed):
    return datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(synth.face_crops_u8(n, seed=seed),
                                                                  synth.mel_windows(n, seed=seed)))


def test_generator_matches_reference_golden(golden, cuda):
    G, _ = _load(amd_models.Wav2Lip(), 0, cuda)
    img, mel = _gen_inputs(2, 1)
    y = G(torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda))
    assert y.shape == (2, 3, 96, 96) and y.is_contiguous()
    err = np.abs(y.cpu().numpy() - golden["gen_out_b2"]).max()
    assert err <= TOL, err


def test_generator_5d_matches_reference_golden(golden, cuda):
    G, _ = _load(amd_models.Wav2Lip(), 0, cuda)
    img, mel = _gen_inputs(2, 1)
    img5 = torch.from_numpy(img).unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous().to(cuda)
    mel5 = torch.from_numpy(mel).unsqueeze(0).to(cuda)
    y5 = G(mel5, img5)
    assert y5.shape == (1, 3, 2, 96, 96)
    assert np.abs(y5.cpu().numpy() - golden["gen_out_5d"]).max() <= TOL


def test_generator_batch128_consistent_with_oracle(cuda):
    """BASELINE config 2 size: every frame of a 128-batch equals the oracle on that frame (first/last/middle
    checked on CPU, all frames checked for batch-invariance against a batch-4 HIP run)."""
    G, sd = _load(amd_models.Wav2Lip(), 0, cuda)
    img, mel = _gen_inputs(128, 5)
    y = G(torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda)).cpu()
    pick = [0, 63, 127]
    ref = models_ref.wav2lip_forward(sd, torch.from_numpy(mel[pick]), torch.from_numpy(img[pick]))
    assert (y[pick] - ref).abs().max() <= TOL
    for lo in range(0, 128, 32):
        ys = G(torch.from_numpy(mel[lo:lo + 4]).to(cuda), torch.from_numpy(img[lo:lo + 4]).to(cuda)).cpu()
        assert (ys - y[lo:lo + 4]).abs().max() <= 2e-5
    assert not torch.isnan(y).any() and y.min() > 0 and y.max() < 1


def test_generator_full_baseline_batch_against_the_oracle(cuda):
    """BASELINE configs[1] in full: ALL 128 frames of the batch against the CPU oracle (round 2 checked 3 of them and compared
    the rest with the HIP path itself), fp32 L-inf and the uint8 frames the reference would write (inference.py:265,269:
    x255., astype(uint8) truncation).  The tune table picks other kernels at N=128 than at small N, so this is the check of the
    configuration the bench line runs."""
    G, sd = _load(amd_models.Wav2Lip(), 0, cuda)
    img, mel = _gen_inputs(128, 5)
    y = G(torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda)).cpu()
    with torch.no_grad():
        ref = torch.cat([models_ref.wav2lip_forward(sd, torch.from_numpy(mel[lo:lo + 16]), torch.from_numpy(img[lo:lo + 16]))
                         for lo in range(0, 128, 16)])
    per_frame = (y - ref).abs().flatten(1).max(dim=1).values
    linf = float(per_frame.max())
    got_u8 = datagen_ref.frames_to_u8(y.numpy())
    ref_u8 = datagen_ref.frames_to_u8(ref.numpy())
    mism = int((got_u8 != ref_u8).sum())
    worst = int(np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32)).max())
    msg = "fp32 L-inf %.3g (worst frame %d), uint8: %d of %d bytes differ, by at most %d" % (
        linf, int(per_frame.argmax()), mism, got_u8.size, worst)
    print(msg)
    assert linf <= TOL, msg                                  # north star: 1e-3
    assert worst <= 1 and mism <= got_u8.size // 10000, msg  # truncation edges only: <= 0.01 % of the bytes, one level


@pytest.mark.parametrize("n", [3, 5, 12, 37])
def test_batches_outside_the_launch_table_run_the_committed_plan_lists(cuda, n):
    """a batch size the tune table does not hold runs the per-plan launch list committed in wav2lip_amd/plan_configs.json (its
    own for 2..7, else the next listed batch size's: engine.apply_plan_configs) - every launch resolves to exactly that
    (configuration, split-K), and every frame still equals the oracle"""
    from wav2lip_amd import engine
    assert engine.plan_configs_enabled()
    src = engine.plan_config_source("generator_96", n)
    assert src == {3: 3, 5: 5, 12: 16, 37: 64}[n]
    want = engine.load_plan_configs()["generator_96"]["plans"][src]
    G, sd = _load(amd_models.Wav2Lip(), 0, cuda)
    got = G.graph(n, 96, 96, cuda).plan.resolved()
    assert [(name, c, k) for name, _, _, (c, k) in got] == [tuple(e) for e in want]
    img, mel = _gen_inputs(n, 11)
    y = G(torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda)).cpu()
    pick = sorted({0, n // 2, n - 1})
    ref = models_ref.wav2lip_forward(sd, torch.from_numpy(mel[pick]), torch.from_numpy(img[pick]))
    assert (y[pick] - ref).abs().max() <= TOL


def test_every_configuration_id_resolves_exactly_where_the_tune_predicate_accepts_it(cuda):
    """the launcher's dry run and w2l_tune_entry_applicable share one shape rule: on every fp32 launch of the batch-128 generator
    plan, forcing configuration id c resolves to c exactly when the launch's tune key accepts c - else a table entry could name a
    kernel that never runs.  The key carries no activation: a sigmoid layer would be the one exception (the plan has none)."""
    import ctypes as C
    from wav2lip_amd import _lib
    lib = _lib.load()
    nk = lib.w2l_tune_key_ints()
    G, _ = _load(amd_models.Wav2Lip(), 0, cuda)
    plan = G.graph(128, 96, 96, cuda).plan
    n = len(plan.records)
    assert not any(layer.geom.act == _lib.ACT_SIGMOID for _, layer, _, _, _ in plan.records)
    disagree = []
    for cid in range(lib.w2l_conv_num_tiles()):
        for i in range(n):
            plan.set_config(i, cid, 1)
        got = plan.resolved()
        for i, (name, layer, N, H, W) in enumerate(plan.records):
            key = layer.tune_key(N, H, W, has_res=plan.has_res[i])
            if (got[i][3][0] == cid) != bool(lib.w2l_tune_entry_applicable((C.c_int * nk)(*key), cid)):
                disagree.append((name, cid, got[i][3]))
    assert n >= 40 and not disagree, disagree


def test_oversized_inference_batch_is_chunked(cuda):
    """a batch larger than one static plan may hold (2 GiB per NHWC buffer: 728 frames at 96x96; plans are capped at
    Wav2Lip.MAX_PLAN_BATCH) runs as chunks, through forward() and through the uint8 runner, with the per-frame results of a
    small-batch run"""
    from wav2lip_amd.inference import Wav2LipRunner
    G, sd = _load(amd_models.Wav2Lip(), 0, cuda)
    old = amd_models.Wav2Lip.MAX_PLAN_BATCH
    amd_models.Wav2Lip.MAX_PLAN_BATCH = 5         # force the chunked route without allocating gigabytes
    try:
        img, mel = _gen_inputs(12, 9)
        y = G(torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda)).cpu()
        assert y.shape == (12, 3, 96, 96)
        ref = models_ref.wav2lip_forward(sd, torch.from_numpy(mel[[0, 5, 11]]), torch.from_numpy(img[[0, 5, 11]]))
        assert (y[[0, 5, 11]] - ref).abs().max() <= TOL
        faces = synth.face_crops_u8(12, seed=4)
        mw = synth.mel_windows(12, seed=4)
        runner = Wav2LipRunner(G, batch_size=12)
        u8 = runner.run_batch(torch.from_numpy(faces).to(cuda), torch.from_numpy(mw).to(cuda)).cpu().numpy()
        one = Wav2LipRunner(G, batch_size=3).run_batch(torch.from_numpy(faces[9:12]).to(cuda), torch.from_numpy(mw[9:12]).to(cuda))
        assert u8.shape == (12, 96, 96, 3) and int(np.abs(u8[9:12].astype(np.int32) - one.cpu().numpy().astype(np.int32)).max()) <= 1
    finally:
        amd_models.Wav2Lip.MAX_PLAN_BATCH = old


def test_generator_repacks_when_weights_change(cuda):
    G, sd = _load(amd_models.Wav2Lip(), 0, cuda)
    img, mel = _gen_inputs(1, 2)
    a, f = torch.from_numpy(mel).to(cuda), torch.from_numpy(img).to(cuda)
    y0 = G(a, f).cpu()
    sd2 = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=9)
    G.load_state_dict(sd2)
    y1 = G(a, f).cpu()
    ref = models_ref.wav2lip_forward(sd2, torch.from_numpy(mel), torch.from_numpy(img))
    assert (y1 - ref).abs().max() <= TOL and (y1 - y0).abs().max() > 1e-3


def test_syncnet_matches_reference_golden(golden, cuda):
    S, sd = _load(amd_models.SyncNet_color(), 2, cuda)
    sm = torch.from_numpy(synth.mel_windows(2, seed=3)).unsqueeze(1)
    sf = torch.from_numpy(synth.sync_faces(2, seed=3))
    a, v = S(sm.to(cuda), sf.to(cuda))
    assert a.shape == (2, 512) and v.shape == (2, 512)
    assert np.abs(a.cpu().numpy() - golden["sync_audio_emb"]).max() <= 1e-5
    assert np.abs(v.cpu().numpy() - golden["sync_face_emb"]).max() <= 1e-5


def test_syncnet_loss_batch64(cuda):
    from wav2lip_amd.losses import cosine_loss
    S, sd = _load(amd_models.SyncNet_color(), 2, cuda)
    n = 64
    sm = torch.from_numpy(synth.mel_windows(n, seed=4)).unsqueeze(1)
    sf = torch.from_numpy(synth.sync_faces(n, seed=4))
    y = torch.from_numpy((np.arange(n) % 2).astype(np.float32)).unsqueeze(1)
    a, v = S(sm.to(cuda), sf.to(cuda))
    loss = cosine_loss(a, v, y.to(cuda)).item()
    ao, vo = models_ref.syncnet_forward(sd, sm, sf)
    ref = models_ref.cosine_loss(ao, vo, y).item()
    assert (a.cpu() - ao).abs().max() <= 1e-5 and (v.cpu() - vo).abs().max() <= 1e-5
    assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref))


def test_disc_matches_reference_golden(golden, cuda):
    D, sd = _load(amd_models.Wav2Lip_disc_qual(), 4, cuda)
    df = torch.from_numpy(synth.disc_frames(1, 2, seed=5))
    p = D(df.to(cuda))
    assert p.shape == (2, 1)
    assert np.abs(p.cpu().numpy() - golden["disc_pred"]).max() <= 1e-5
    loss = D.perceptual_forward(df.to(cuda)).item()
    ref = torch.nn.functional.binary_cross_entropy(torch.from_numpy(golden["disc_pred"]), torch.ones(2, 1)).item()
    assert abs(loss - ref) <= 1e-5


def test_train_mode_single_sample_raises_like_torch(cuda):
    """train-mode BatchNorm over one value per channel (the 1x1 bottleneck at batch 1): torch raises ValueError, so do we"""
    G = amd_models.Wav2Lip().to(cuda).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        G(torch.zeros(1, 1, 80, 16, device=cuda), torch.zeros(1, 6, 96, 96, device=cuda))


def test_train_mode_forward_uses_batch_statistics(cuda):
    """model.train() under no_grad still runs BN on batch statistics (and updates the running ones), as nn.BatchNorm2d"""
    from wav2lip_amd import synthetic as synth
    G = amd_models.Wav2Lip()
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0)
    G.load_state_dict(sd)
    G = G.to(cuda).train()
    faces = torch.rand(3, 6, 96, 96)
    mels = torch.rand(3, 1, 80, 16) * 8 - 4
    with torch.no_grad():
        y = G(mels.to(cuda), faces.to(cuda)).cpu()
    ref_sd = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        ref = models_ref.wav2lip_graph(ref_sd, mels, faces, training=True)
    assert (y - ref).abs().max().item() <= 1e-4
    rv = G.state_dict()["face_encoder_blocks.0.0.conv_block.1.running_var"].cpu()
    assert (rv - ref_sd["face_encoder_blocks.0.0.conv_block.1.running_var"]).abs().max().item() <= 1e-5
    assert not torch.equal(rv, sd["face_encoder_blocks.0.0.conv_block.1.running_var"])


def test_lse_like_scores_match_the_cpu_scoring(cuda):
    """BASELINE metric's parity half: the LSE-D / LSE-C scoring arithmetic of evaluation/scores_LSE on the in-tree
    SyncNet_color embeddings, engine frames + HIP scoring vs oracle frames + the reference's torch expressions"""
    from oracle import audio_ref, lse_ref
    from wav2lip_amd import audio, evaluation
    from wav2lip_amd.inference import Wav2LipRunner, mel_chunk_starts
    G, sdg = _load(amd_models.Wav2Lip(), 0, cuda)
    S, sds = _load(amd_models.SyncNet_color(), 2, cuda)
    wav = synth.noise_wav(16000 * 2, seed=31)
    mel_ref = audio_ref.melspectrogram(wav)
    starts = mel_chunk_starts(mel_ref.shape[1], 25.)[:24]
    n = len(starts)
    faces = synth.face_crops_u8(n, seed=32)
    mel_dev = audio.melspectrogram_device(wav, cuda)
    runner = Wav2LipRunner(G, batch_size=n)
    out = runner.run_batch(torch.from_numpy(faces).to(cuda), mel=mel_dev,
                           starts=torch.tensor(starts, dtype=torch.int32, device=cuda)).clone()
    got = evaluation.lse_like(S, out, mel_dev, vshift=3)       # 20 windows: keep most offsets inside the clip
    # CPU pipeline: oracle mel windows -> oracle generator -> uint8 frames -> oracle SyncNet -> reference scoring
    mw = np.stack([mel_ref[:, s:s + 16] for s in starts])
    img, mel = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(faces, mw))
    ref_frames = datagen_ref.frames_to_u8(models_ref.wav2lip_forward(sdg, torch.from_numpy(mel), torch.from_numpy(img)).numpy())
    off, conf, minval, mdist = lse_ref.lse_like(sds, ref_frames, mel_ref, vshift=3)
    assert got["n"] == len(ref_frames) - 4
    two = np.sort(mdist.numpy())[:2]
    assert got["offset"] == off or two[1] - two[0] <= 2e-3       # argmin only compared when it is not a near-tie
    assert abs(got["lse_d"] - minval) <= 1e-3 and abs(got["lse_c"] - conf) <= 1e-3
    assert np.abs(got["mdist"] - mdist.numpy()).max() <= 1e-3
