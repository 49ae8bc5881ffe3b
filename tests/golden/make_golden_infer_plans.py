"""Records what the three inference graphs (generator, SyncNet, S3FD) build and compute, per storage precision, at one small
size each: the launch lists with their shapes and resolved configurations, the buffer layouts, and the output bytes.  Outputs are
bit-reproducible across processes and boxes while W2L_AUTOTUNE is unset (wav2lip_amd/engine.py), so the file this writes on one
commit is an exact reference for a later one that must not change behaviour: tests/test_infer_plans_gpu.py calls `collect` again
and compares with ==.  Needs a HIP device.

    python tests/golden/make_golden_infer_plans.py          # writes tests/golden/golden_infer_plans_v1.npz

golden_infer_plans_v1.npz was written on the commit BEFORE the per-network fp32 / bf16 graph classes were merged into one class
per network.  Re-running this on a later tree turns the fixture into a record of that tree: do it only for a change that is meant
to alter launches or bytes, and say so.

Weights are wav2lip_amd.synthetic's (seed 0), inputs its seeded generators.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from wav2lip_amd import synthetic as synth  # noqa: E402

PRECISIONS = ("f32", "bf16")
PATH = os.path.join(HERE, "golden_infer_plans_v1.npz")
MEL_STARTS = (0, 37, 84)            # ragged window starts in a 100-column spectrogram; the last window ends at its last column


def _seeded(model):
    model.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=0))
    return model


def _layout(t):
    return [list(t.shape), str(t.dtype), list(t.stride())]


def _records(plan):
    return [[name, N, H, W] for name, _, N, H, W in plan.records]


def _resolved(plan):
    return [[name, flops, family, list(cfg)] for name, flops, family, cfg in plan.resolved()]


def _plan_buffers(plan):
    """layout of every NHWC buffer the plan's launches read or write, in the order the launches first name them: the inputs, the
    scratch buffers, every concat buffer and the output"""
    seen, out = set(), []
    for t in plan.keep:
        if isinstance(t, torch.Tensor) and t.dim() == 4 and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append(_layout(t))
    return out


def _act(a):
    return [a.N, a.H, a.W, a.C, a.cs, a.off]


def _table(dtype, entries, cuda):
    t = np.zeros(len(entries), dtype)
    for i, e in enumerate(entries):
        t[i] = e
    return torch.from_numpy(t.view(np.uint8)).to(cuda)


def generator(cuda, precision, out):
    """N=3 at 96x96: a batch the launch table does not hold, so the fp32 plan takes its configurations from plan_configs.json"""
    from wav2lip_amd import models, multiclip
    from wav2lip_amd.inference import Wav2LipRunner
    G = _seeded(models.Wav2Lip()).to(cuda).eval()
    runner = Wav2LipRunner(G, batch_size=3, precision=precision)
    faces = torch.from_numpy(synth.face_crops_u8(3, seed=7)).to(cuda)
    spec = torch.from_numpy(np.random.default_rng(11).uniform(-4.0, 4.0, (80, 100)).astype(np.float32)).to(cuda)
    windows = torch.stack([spec[:, s:s + 16] for s in MEL_STARTS]).contiguous()
    starts = torch.tensor(MEL_STARTS, dtype=torch.int32, device=cuda)
    rows = _table(multiclip.MEL_ROW, [(spec.data_ptr(), spec.shape[1], s) for s in MEL_STARTS], cuda)
    frames = {}
    frames["windows"] = runner.run_batch(faces, mel_windows=windows).cpu().numpy().copy()
    pred = runner.last_pred_nchw().cpu().numpy()
    frames["starts"] = runner.run_batch(faces, mel=spec, starts=starts).cpu().numpy().copy()
    frames["rows"] = runner.run_batch(faces, mel_rows=rows).cpu().numpy().copy()
    g = G.graph(3, 96, 96, cuda, precision=precision)
    meta = {"records": _records(g.plan), "has_res": [bool(r) for r in g.plan.has_res], "resolved": _resolved(g.plan),
            "n_face": g.n_face, "n_audio": g.n_audio, "scratch_bytes": g.scratch_bytes, "x_in": _layout(g.x_in),
            "mel_in": _layout(g.mel_in), "buffers": _plan_buffers(g.plan), "pred_sha256": hashlib.sha256(pred.tobytes()).hexdigest(),
            "pred": [list(pred.shape), str(pred.dtype)]}
    if precision == "bf16":
        meta["dispatch"] = [list(d) for d in g.dispatch()]
    out["gen_%s_meta" % precision] = np.array(json.dumps(meta))
    out["gen_%s_frames" % precision] = frames["windows"]
    return frames


def syncnet(cuda, precision, out):
    """N=2 at 48x96: windows 0 and 1 of six crops, through `forward` and through `embed_rows` on a row table of the same windows"""
    from wav2lip_amd import evaluation, models
    S = _seeded(models.SyncNet_color()).to(cuda).eval()
    crops = synth.face_crops_u8(6, seed=5)
    x = torch.from_numpy(crops)[:, 48:].permute(0, 3, 1, 2).float() / 255.
    faces = torch.stack([x[v:v + 5].reshape(15, 48, 96) for v in range(2)]).contiguous().to(cuda)
    mels = torch.from_numpy(synth.mel_windows(2, seed=5)).unsqueeze(1).contiguous().to(cuda)
    a, v = S(mels, faces, precision=precision)
    crops_dev = torch.from_numpy(crops).to(cuda)
    spec = mels[:, 0].permute(1, 0, 2).reshape(80, 2 * 16).contiguous()
    rows = _table(evaluation.SYNC_ROW, [(crops_dev.data_ptr() + k * 96 * 96 * 3, spec.data_ptr(), spec.shape[1], 16 * k, (0, 0))
                                        for k in range(2)], cuda)
    a2 = torch.full((2, 512), float("nan"), device=cuda)
    v2 = torch.full((2, 512), float("nan"), device=cuda)
    S.embed_rows(rows, 2, a2, v2, precision=precision)
    g = S._eval_graph(2, 48, 96, cuda, precision)
    meta = {"records": _records(g.plan), "has_res": [bool(r) for r in g.plan.has_res], "resolved": _resolved(g.plan),
            "face_in": _layout(g.face_in), "mel_in": _layout(g.mel_in), "face_out": _act(g.face_out), "audio_out": _act(g.audio_out),
            "buffers": _plan_buffers(g.plan)}
    if precision == "bf16":
        meta["dispatch"] = [list(d) for d in g.dispatch()]
        meta["scratch_bytes"] = g.scratch_bytes
    out["sync_%s_meta" % precision] = np.array(json.dumps(meta))
    out["sync_%s_audio" % precision] = a.cpu().numpy()
    out["sync_%s_face" % precision] = v.cpu().numpy()
    return {"forward": (a.cpu().numpy(), v.cpu().numpy()), "rows": (a2.cpu().numpy(), v2.cpu().numpy())}


def _op(op):
    if op[0] == "convs":
        return ["convs", _records(op[1]), _resolved(op[1]), _plan_buffers(op[1])]
    if op[0] == "pool":
        return ["pool", _act(op[1]), _act(op[2])]
    if op[0] == "l2norm":
        return ["l2norm", _act(op[1]), list(op[2].shape), _act(op[3])]
    return ["head", [op[1].cin, op[1].ncls], _act(op[2]), op[3], list(op[4].shape)]


def s3fd(cuda, precision, out):
    """B=1 at 64x72 (non-square, just above MIN_FRAME): `dense_boxes`, `dense_boxes_rows` at det_scale 1, and at det_scale 2 on a
    128x144 frame (the same graph)"""
    from wav2lip_amd import face_detection
    net = face_detection.s3fd()
    net.load_state_dict(synth.s3fd_state_dict())
    net = net.to(cuda).eval()
    small = torch.from_numpy(synth.s3fd_frames(seed=1, B=1, H=64, W=72)).to(cuda)
    big = torch.from_numpy(synth.s3fd_frames(seed=1, B=1, H=128, W=144)).to(cuda)
    tables = {}
    tables["dense"] = [t.cpu().numpy().copy() for t in net.dense_boxes(small, precision=precision)]
    g = net._graph(1, 64, 72, cuda, precision)
    for key, img, k in (("rows", small, 1), ("rows2", big, 2)):
        addr = torch.tensor([img.data_ptr()], dtype=torch.int64, device=cuda)
        tables[key] = [t.cpu().numpy().copy() for t in net.dense_boxes_rows(addr, 1, img.shape[1], img.shape[2], precision, k)]
        assert net._graph(1, 64, 72, cuda, precision) is g
    meta = {"ops": [_op(op) for op in g.ops], "x_in": _layout(g.x_in), "dense": [list(t.shape) for t in g.dense]}
    if precision == "bf16":
        meta["resolved"] = [list(r) for r in g.resolved()]
        meta["dispatch"] = [list(d) for d in g.dispatch()]
    else:
        meta["levels"] = [[_act(conf), _act(loc), ncls, stride] for conf, loc, ncls, stride in g.levels]
    out["s3fd_%s_meta" % precision] = np.array(json.dumps(meta))
    for key, ts in tables.items():
        for i, t in enumerate(ts):
            out["s3fd_%s_%s_%d" % (precision, key, i)] = t
    return tables


def collect(cuda):
    """({fixture key: array}, {what each network's other doors gave}) of the tree this runs on"""
    out, doors = {}, {}
    for p in PRECISIONS:
        doors["gen_" + p] = generator(cuda, p, out)
        doors["sync_" + p] = syncnet(cuda, p, out)
        doors["s3fd_" + p] = s3fd(cuda, p, out)
    return out, doors


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    assert os.environ.get("W2L_AUTOTUNE", "0") != "1", "stopwatch tuning makes the bytes differ from run to run"
    out, doors = collect(torch.device("cuda:0"))
    dest = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(dest, **out)
    print("wrote", dest, os.path.getsize(dest), "bytes")
    for p in PRECISIONS:
        f = doors["gen_" + p]
        assert f["windows"].tobytes() == f["starts"].tobytes() == f["rows"].tobytes(), "generator %s: the audio forms differ" % p
        s = doors["sync_" + p]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(s["forward"], s["rows"])), "SyncNet %s: embed_rows differs" % p
        print(p, "generator frames", f["windows"].shape, "mean", float(f["windows"].mean()),
              "sync |a|", float(np.abs(s["forward"][0]).sum()), "s3fd max score", max(float(t[..., 4].max()) for t in doors["s3fd_" + p]["dense"]))


if __name__ == "__main__":
    main()
