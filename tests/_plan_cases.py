"""Cases for the fp32 generator plans (tests/test_plan_cases_cpu.py, tests/test_infer_f32_plans_gpu.py): which batch sizes to
run, which (record, configuration id, split-K) list each of them must resolve to, and one pool of frames with its CPU oracle.

Host only: numpy, json, the committed launch files and the library's host-side entry points (w2l_conv_out_hw); no device.

Which list a batch size N runs (wav2lip_amd/engine.py): a size of plan_configs.json's "table" resolves every launch through the
shape-keyed table (tune_table.json) under the launch's tune key; any other N runs the list of `engine.plan_config_source` - its
own for 2..7, else the next listed size's, the largest one's beyond that; batches above Wav2Lip.MAX_PLAN_BATCH run as chunks."""
import ctypes as C
import functools
import json

import numpy as np

KIND = "generator_96"
POOL = 32
CHUNK_EXTRA = 88          # the one chunked size is MAX_PLAN_BATCH + 88


def max_plan_batch():
    from wav2lip_amd import models
    return models.Wav2Lip.MAX_PLAN_BATCH


def plan_doc():
    from wav2lip_amd import engine
    return engine.load_plan_configs()[KIND]


def source(N):
    """what decides the launches of an N-frame plan: ("table", N) or ("list", M), M the batch size whose committed list N runs"""
    from wav2lip_amd import engine
    src = engine.plan_config_source(KIND, N)
    return ("table", N) if src is None else ("list", src)


def borrowers(M):
    """every N in 1..MAX_PLAN_BATCH that runs the committed list of batch size M"""
    return [n for n in range(1, max_plan_batch() + 1) if source(n) == ("list", M)]


def _runs(ns):
    """maximal runs of consecutive integers in the sorted list `ns` as (first, last)"""
    out = []
    for n in ns:
        if out and n == out[-1][1] + 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return [tuple(r) for r in out]


def sizes():
    """the batch sizes to run, from the two committed files alone: every size of the "table" list; every size with a list of its
    own; for every list the smallest and the largest N of each run of consecutive sizes in 1..MAX_PLAN_BATCH that borrow it (a
    table size in between cuts a range in two: 129..255 and 257..512 both run the 256 list); MAX_PLAN_BATCH itself with the odd
    size just under it; and one chunked size, MAX_PLAN_BATCH + 88"""
    d = plan_doc()
    cap = max_plan_batch()
    out = set(d["table"]) | set(d["plans"])
    for M in d["plans"]:
        for lo, hi in _runs(borrowers(M)):
            out |= {lo, hi}
    out |= {cap - 1, cap, cap + CHUNK_EXTRA}
    return sorted(out)


def chunks(N):
    cap = max_plan_batch()
    return [min(cap, N - lo) for lo in range(0, N, cap)]


@functools.lru_cache(maxsize=None)
def launches():
    """[(record name, the 14 leading ints of its tune key, H, W)] of the generator plan at 96x96, in launch order, from the
    module tree alone (models/wav2lip.py:_GeneratorGraph records them in this order): key = transposed cin cout kh kw sh sw ph pw
    oph opw precision has_residual head_c (then N H W)"""
    from wav2lip_amd import _lib, models
    from wav2lip_amd._lib import ACT_RELU
    from wav2lip_amd.bf16 import conv_geom
    lib = _lib.load()
    G = models.Wav2Lip()
    out = []

    def chain(name, blocks, h, w, head_c=0):
        for j, blk in enumerate(blocks):
            g = conv_geom(blk.conv_block[0], blk._transposed, ACT_RELU)
            key = (g.transposed, g.cin, g.cout, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.oph, g.opw, 0, int(blk.residual), head_c)
            out.append(("%s.%d" % (name, j), key, h, w))
            ho, wo = C.c_int(), C.c_int()
            assert lib.w2l_conv_out_hw(C.byref(g), h, w, C.byref(ho), C.byref(wo)) == 0
            h, w = ho.value, wo.value
        return h, w

    h, w = 96, 96
    for i, blk in enumerate(G.face_encoder_blocks):
        h, w = chain("face_encoder_blocks.%d" % i, blk, h, w)
    h, w = chain("audio_encoder", G.audio_encoder, 80, 16)
    for i, blk in enumerate(G.face_decoder_blocks):
        h, w = chain("face_decoder_blocks.%d" % i, blk, h, w)      # the skip concat adds channels, not pixels
    chain("output_block", [G.output_block[0]], h, w, head_c=G.output_block[1].out_channels)
    return tuple(out)


def tune_keys(N):
    """[(record name, 17-int tune key)] of the N-frame plan"""
    return [(name, key + (N, h, w)) for name, key, h, w in launches()]


@functools.lru_cache(maxsize=None)
def table_entries(path=None):
    """{17-int key: (configuration id, split-K)} of a tune-table file (the committed default table when `path` is None)"""
    from wav2lip_amd import _lib
    with open(path or _lib.TUNE_TABLE_PATH) as fh:
        doc = json.load(fh)
    nk = doc["key_ints"]
    return {tuple(e[:nk]): (int(e[nk]), int(e[nk + 1])) for e in doc["entries"]}


def expected_plan(N):
    """the [(record, id, split-K)] an N-frame plan (N <= MAX_PLAN_BATCH) must resolve to: the table's entries under the plan's tune
    keys for a table size (a KeyError names a launch the table does not hold), else the committed list N borrows"""
    kind, M = source(N)
    if kind == "table":
        tab = table_entries()
        return [(name,) + tab[key] for name, key in tune_keys(N)]
    return [(name, int(c), int(k)) for name, c, k in plan_doc()["plans"][M]]


def expected(N):
    """`expected_plan` of the LAST plan an N-frame batch runs (the whole batch up to MAX_PLAN_BATCH, else its last chunk)"""
    return expected_plan(chunks(N)[-1])


def source_id(N):
    """readable name of what decides the launches of an N-frame batch, e.g. "table128", "list64", "list256+list128" """
    names = []
    for n in chunks(N):
        name = "%s%d" % source(n)
        if not names or names[-1] != name:
            names.append(name)
    return "+".join(names)


def by_source():
    """{source id: [sizes of `sizes()` it decides]} in ascending order of the first size"""
    out = {}
    for n in sizes():
        out.setdefault(source_id(n), []).append(n)
    return out


def all_expected_launches():
    """every (record, id, split-K) that some plan of 1..MAX_PLAN_BATCH frames may be asked to run: the table's generator entries
    at the table sizes and every list some size borrows"""
    want = set()
    for n in range(1, max_plan_batch() + 1):
        if source(n) == ("table", n) or n in plan_doc()["plans"]:
            want |= set(expected_plan(n))
    for M in plan_doc()["plans"]:
        if borrowers(M):
            want |= {(name, int(c), int(k)) for name, c, k in plan_doc()["plans"][M]}
    return want


def frames_u8(pred):
    """uint8 frames [n,96,96,3] of a prediction [n,3,96,96] (tensor or array) in its own precision: x 255, truncated"""
    from oracle import datagen_ref
    return datagen_ref.frames_to_u8(np.asarray(pred))


def u8_diff(a, b):
    """(bytes that differ, worst difference in levels)"""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int((d != 0).sum()), int(d.max())


@functools.lru_cache(maxsize=None)
def pool(P=POOL):
    """P frames and their CPU references under the seed-0 synthetic weights: {"faces" uint8 [P,96,96,3], "mels" float32 [P,80,16],
    "img" / "mel" the model inputs of datagen_ref, "ref64" the oracle models_ref.wav2lip_forward in float64, "ref32" the same
    forward in torch float32 (both [P,3,96,96], run in chunks of 8), "u8_64" / "u8_32" their uint8 frames, "d32" the L-inf distance
    between the two}.  Input j of an N-frame batch is pool frame j mod P, so one oracle run serves every size.  Callers must not
    write into the arrays."""
    import torch
    from oracle import datagen_ref, models_ref
    from wav2lip_amd import models
    from wav2lip_amd import synthetic as synth
    shapes = {k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}
    sd = synth.synthetic_state_dict(shapes, seed=0)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    faces, mels = synth.face_crops_u8(P, seed=5), synth.mel_windows(P, seed=5)
    img, mel = datagen_ref.to_model_inputs(*datagen_ref.datagen_batch(faces, mels))
    ti, tm = torch.from_numpy(img), torch.from_numpy(mel)
    with torch.no_grad():
        ref64 = torch.cat([models_ref.wav2lip_forward(sd64, tm[lo:lo + 8].double(), ti[lo:lo + 8].double()) for lo in range(0, P, 8)])
        ref32 = torch.cat([models_ref.wav2lip_forward(sd, tm[lo:lo + 8], ti[lo:lo + 8]) for lo in range(0, P, 8)])
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    return {"faces": faces, "mels": mels, "img": img, "mel": mel, "sd": sd, "ref64": ref64, "ref32": ref32,
            "u8_64": frames_u8(ref64.numpy()), "u8_32": frames_u8(ref32.numpy()),
            "d32": float((ref32.double() - ref64).abs().max())}


def batch_index(N, P=POOL):
    return np.arange(N) % P
