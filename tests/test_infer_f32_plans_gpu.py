"""The default fp32 inference path of the generator at every batch size tests/_plan_cases.py derives from the committed launch
files (tune_table.json, plan_configs.json): the sizes of the launch table, the sizes with a list of their own, both ends of every
range of sizes that borrow a list, MAX_PLAN_BATCH and one chunked batch - and the load-time switches W2L_EXACT, W2L_SPLIT,
W2L_TUNE_TABLE and W2L_PLAN_CONFIGS in fresh processes.

Input j of a batch is pool frame j mod 32 (face_crops_u8 / mel_windows, seed 5; seed-0 synthetic weights), so one float64 oracle
run (oracle.models_ref.wav2lip_forward, about 6 s of CPU) serves every size.  Every size is held to:

  launch list     plan.resolved() is exactly the (record, id, split-K) list `_plan_cases.expected(N)` derives from the files;
  1e-4            every frame within the project's bar of the float64 oracle;
  16 x d32        every frame within 16 x d32 of it, d32 = L-inf between the SAME forward in torch float32 and in float64 on the
                  pool (measured by the test on the CPU, from the reference alone).  What the default path adds over a plain float32
                  graph - F(4x4) Winograd transforms, fp32 operands as three bf16 pieces - has to fit that margin; it is twenty
                  times tighter than 1e-4;
  uint8 frames    the runner's frames are datagen_ref.frames_to_u8 of its own prediction and differ from the oracle's frames in at
                  most 0.01 % of the bytes, by one level;
  position        frames j and j - 32 of one plan have identical inputs and must be bit-identical (tile masking, split-K
                  workspaces, F(4x4) tile blocks that run across image boundaries are what would break it);
  same launches   two sizes whose resolved lists are identical agree bit for bit on the frames they share.

Measured on an MI355X, d32 = 3.014e-07 (3.005e-07 on another CPU), so the bars are 1e-4 and 16 x d32 = 4.8e-06; no size needed an
exception, the worst is 2.60 x d32.  uint8 = bytes that differ from the float64 oracle's frames, all by one level (bar 0.01 %).

     N  source            L-inf      x d32  uint8
     1  table1            1.741e-07   0.58  0/27648
     2  list2             2.134e-07   0.71  0/55296
     3  list3             2.256e-07   0.75  1/82944
     4  list4             3.143e-07   1.04  2/110592
     5  list5             2.394e-07   0.79  1/138240
     6  list6             2.608e-07   0.87  1/165888
     7  list7             2.632e-07   0.87  2/193536
     8  table8            2.641e-07   0.88  2/221184
     9  list16            5.995e-07   1.99  2/248832
    15  list16            5.995e-07   1.99  3/414720
    16  table16           5.995e-07   1.99  3/442368
    17  list32            5.011e-07   1.66  7/470016
    31  list32            5.178e-07   1.72  13/857088
    32  table32           5.224e-07   1.73  13/884736
    33  list64            7.217e-07   2.39  15/912384
    63  list64            7.217e-07   2.39  30/1741824
    64  table64           7.217e-07   2.39  30/1769472
    65  list128           7.825e-07   2.60  38/1797120
   127  list128           7.825e-07   2.60  74/3511296
   128  table128          7.825e-07   2.60  76/3538944
   129  list256           7.392e-07   2.45  68/3566592
   255  list256           7.392e-07   2.45  135/7050240
   256  table256          7.392e-07   2.45  136/7077888
   257  list256           7.392e-07   2.45  136/7105536
   511  list256           7.392e-07   2.45  271/14128128
   512  list256           7.392e-07   2.45  272/14155776
   600  list256+list128   7.825e-07   2.60  320/16588800

  (600: all frames through forward(); the runner's last 88 alone are 7.825e-07.)  Sizes of one source whose worst frame is among
  the frames they share print the same figure: they are bit-identical on those frames (thirteen pairs compared).

  switch (fresh process)                      N=8             N=37            N=128           (L-inf, x d32)
  W2L_EXACT=1 (bar 8 x d32)                   2.758e-07 0.92  4.196e-07 1.39  4.292e-07 1.42
  W2L_SPLIT=0                                 2.547e-07 0.84  6.765e-07 2.24  7.600e-07 2.52
  W2L_TUNE_TABLE=tune_table_one_in_flight     2.641e-07 0.88  4.196e-07 1.39  7.257e-07 2.41
  W2L_TUNE_TABLE=0                            3.326e-07 1.10  4.196e-07 1.39  3.638e-07 1.21
  W2L_PLAN_CONFIGS=0                          2.641e-07 0.88  4.196e-07 1.39  7.825e-07 2.60
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _plan_cases as pc
from conftest import ROOT
from wav2lip_amd import models as amd_models

pytestmark = pytest.mark.gpu
TOL = 1e-4                 # the project's bar on generator pixels
TIGHT = 16                 # x d32: the bar of the default path
TIGHT_EXACT = 8            # x d32: W2L_EXACT=1 (no F(4x4) Winograd)
SOURCES = pc.by_source()
CHUNKED = [s for s, ns in SOURCES.items() if any(n > pc.max_plan_batch() for n in ns)]

_RAN = {}                  # N -> {"resolved": [(record, id, split-K)] per plan it ran, "row": the printed line}
_BY_LAUNCHES = {}          # resolved list -> (N, prediction bits, uint8 frames) of the largest size that ran it
_PAIRS = []                # (N, N') compared bit for bit


@pytest.fixture(scope="module")
def pool(cuda):
    p = dict(pc.pool())
    p["faces_dev"] = torch.from_numpy(p["faces"]).to(cuda)
    p["mels_dev"] = torch.from_numpy(p["mels"]).to(cuda)
    print("d32 = %.3e (torch float32 vs float64, 32 frames); bars: %.1e and %d x d32 = %.3e" % (p["d32"], TOL, TIGHT, TIGHT * p["d32"]))
    return p


@pytest.fixture(scope="module")
def gen(cuda, pool):
    from wav2lip_amd import engine
    assert not engine.AUTOTUNE and engine.plan_configs_enabled(), "this file checks the default configuration"
    G = amd_models.Wav2Lip()
    G.load_state_dict(pool["sd"])
    G = G.to(cuda).eval()
    yield G
    G._graphs.clear()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launches(plan):
    return [(name, c, k) for name, _, _, (c, k) in plan.resolved()]


def _run(G, pool, n):
    """an n-frame batch through a fresh runner with no other plan resident: (uint8 frames [n], prediction of the LAST plan,
    {frames of a plan: its graph})"""
    from wav2lip_amd.inference import Wav2LipRunner
    G._graphs.clear()
    idx = torch.from_numpy(pc.batch_index(n)).to(pool["faces_dev"].device)
    r = Wav2LipRunner(G, batch_size=n)
    u8 = r.run_batch(pool["faces_dev"][idx], pool["mels_dev"][idx]).cpu().numpy().copy()
    y = r.last_pred_nchw().cpu()
    graphs = {k[0]: v[1] for k, v in G._graphs.items()}
    assert sorted(graphs) == sorted(set(pc.chunks(n))), (n, sorted(graphs))
    return u8, y, graphs


def _check_launch_lists(n, graphs):
    """every plan the batch ran resolved to the list the committed files give it, under the tune keys the host-side walk derives"""
    got = []
    for m in pc.chunks(n):
        plan = graphs[m].plan
        keys = [layer.tune_key(N, H, W, has_res=plan.has_res[i]) for i, (_, layer, N, H, W) in enumerate(plan.records)]
        assert [(r[0], k) for r, k in zip(plan.records, keys)] == pc.tune_keys(m), "N=%d: tune keys differ from the host-side walk" % m
        have, want = _launches(plan), pc.expected_plan(m)
        diff = [(h, w) for h, w in zip(have, want) if h != w]
        assert have == want, "N=%d (%s): %d launches resolve to something else than the committed list, first %s" % (
            m, "%s %d" % pc.source(m), len(diff), diff[:3])
        got.append(tuple(have))
    return got


def _check_frames(label, pool, idx, y, u8, tight=TIGHT):
    """prediction `y` of pool frames `idx` and their uint8 frames `u8` against the float64 oracle: per-frame L-inf within 1e-4 and
    within `tight` x d32, the frames the truncation of the prediction and within one level of the oracle's on <= 0.01 % of the
    bytes; returns the printed figures"""
    per_frame = (y.double() - pool["ref64"][idx]).abs().flatten(1).max(dim=1).values
    linf, ratio = float(per_frame.max()), float(per_frame.max()) / pool["d32"]
    mism, worst = pc.u8_diff(u8, pool["u8_64"][idx])
    row = "L-inf %.3e (frame %d) = %.2f x d32, uint8: %d of %d bytes differ, by at most %d" % (
        linf, int(per_frame.argmax()), ratio, mism, u8.size, worst)
    print("%-28s %s" % (label, row))
    assert bool(torch.isfinite(y).all()) and np.array_equal(u8, pc.frames_u8(y.numpy())), label + ": frames are not the truncated prediction"
    assert linf <= TOL, label + ": " + row
    assert linf <= tight * pool["d32"], label + ": " + row
    assert worst <= 1 and mism * 10000 <= u8.size, label + ": " + row
    return row


def _check_positions(n, y, u8, lo=0):
    """frames j and j - 32 of one plan are bit-identical; `y` covers frames lo.. of the batch, `u8` all of them"""
    cap = pc.max_plan_batch()
    pos = np.arange(n)
    dup = pos[pos - pc.POOL >= pos // cap * cap]
    assert np.array_equal(u8[dup], u8[dup - pc.POOL]), "N=%d: uint8 frames with identical inputs differ" % n
    dup = dup[dup - pc.POOL >= lo] - lo
    yb = _bits(y)
    assert torch.equal(yb[dup], yb[dup - pc.POOL]), "N=%d: predictions with identical inputs differ" % n
    return len(dup)


def _compare_same_launches(n, launches, y, u8):
    prev = _BY_LAUNCHES.get(launches)
    if prev is not None:
        m = min(n, prev[0])
        assert torch.equal(_bits(y[:m]), prev[1][:m]) and np.array_equal(u8[:m], prev[2][:m]), \
            "N=%d and N=%d resolve every launch alike but differ on the frames they share" % (prev[0], n)
        _PAIRS.append((prev[0], n))
    if prev is None or prev[0] < n:
        _BY_LAUNCHES[launches] = (n, _bits(y).clone(), u8)


@pytest.mark.parametrize("src", [s for s in SOURCES if s not in CHUNKED])
def test_sizes_of_one_source_list_against_the_oracle(cuda, pool, gen, src):
    """every size of `_plan_cases.sizes()` that one source decides - a table size, a size with its own list, or the ends of the
    ranges that borrow one list (129, 255, 257, 511 and 512 all run the 256 list): launch list, both bars on every frame, uint8
    frames, position independence, and bit-equality with every earlier size that resolved the same launches"""
    for n in SOURCES[src]:
        u8, y, graphs = _run(gen, pool, n)
        (launches,) = _check_launch_lists(n, graphs)
        idx = pc.batch_index(n)
        row = _check_frames("N=%d (%s)" % (n, src), pool, idx, y, u8)
        _check_positions(n, y, u8)
        _compare_same_launches(n, launches, y, u8)
        _RAN[n] = {"resolved": [launches], "row": row}


@pytest.mark.parametrize("src", CHUNKED)
def test_chunked_batch_through_forward_and_the_runner(cuda, pool, gen, src):
    """600 frames run as 512 + 88, through the uint8 runner and through forward(): the first 512 frames equal the 512-frame run bit
    for bit (uint8 frames of the runner, predictions of forward(), and the two doors agree), the last 88 - which run the 128
    list - are within the bars; both plans resolve to their committed lists"""
    cap = pc.max_plan_batch()
    (n,) = SOURCES[src]
    assert pc.chunks(n) == [cap, pc.CHUNK_EXTRA]
    idx = pc.batch_index(n)
    u8, y_last, graphs = _run(gen, pool, n)
    resolved = _check_launch_lists(n, graphs)
    assert y_last.shape[0] == pc.CHUNK_EXTRA
    row = _check_frames("N=%d runner, last %d" % (n, pc.CHUNK_EXTRA), pool, idx[cap:], y_last, u8[cap:])
    _check_positions(n, y_last, u8, lo=cap)
    del graphs
    gen._graphs.clear()
    yf = gen(torch.from_numpy(pool["mel"][idx]).to(cuda), torch.from_numpy(pool["img"][idx]).to(cuda)).cpu()
    assert yf.shape == (n, 3, 96, 96)
    assert sorted(k[0] for k in gen._graphs) == sorted(pc.chunks(n))
    assert torch.equal(_bits(yf[cap:]), _bits(y_last)), "forward() and the runner differ on the last chunk"
    _check_frames("N=%d forward(), all" % n, pool, idx, yf, pc.frames_u8(yf.numpy()))
    assert np.array_equal(u8, pc.frames_u8(yf.numpy()))
    u8_cap, y_cap, graphs = _run(gen, pool, cap)
    assert _check_launch_lists(cap, graphs) == resolved[:1]
    assert np.array_equal(u8[:cap], u8_cap), "the first %d frames of the chunked batch differ from the %d-frame run" % (cap, cap)
    assert torch.equal(_bits(yf[:cap]), _bits(y_cap))
    _RAN[n] = {"resolved": resolved, "row": row}


def test_every_expected_launch_ran_and_enough_sizes_were_compared_bit_for_bit():
    """module-level closing check (runs after the tests above, in file order): every size of the set ran, every (record, id,
    split-K) the CPU test expects was resolved at a size that ran, and at least five pairs of sizes with identical launches were
    compared bit for bit"""
    assert sorted(_RAN) == pc.sizes(), "sizes that did not run: %s" % sorted(set(pc.sizes()) - set(_RAN))
    print("d32 = %.3e" % pc.pool()["d32"])
    for n in sorted(_RAN):
        print("N=%-4d %-20s %s" % (n, pc.source_id(n), _RAN[n]["row"]))
    have = {e for r in _RAN.values() for lst in r["resolved"] for e in lst}
    want = pc.all_expected_launches()
    assert want <= have, sorted(want - have)[:10]
    print("pairs compared bit for bit: %s" % _PAIRS)
    assert len(_PAIRS) >= 5, _PAIRS


# ---------------------------------------------------------------- the load-time switches, one fresh process each
_CHILD = r'''
import json, sys
import numpy as np, torch
root, work = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from wav2lip_amd import _lib, engine, models
from wav2lip_amd import synthetic as synth
from wav2lip_amd.inference import Wav2LipRunner
dev = torch.device("cuda", 0)
G = models.Wav2Lip()
G.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0))
G = G.to(dev).eval()
faces = torch.from_numpy(synth.face_crops_u8(32, seed=5)).to(dev)       # the pool of tests/_plan_cases.py
mels = torch.from_numpy(synth.mel_windows(32, seed=5)).to(dev)
out = {"tune_count": int(_lib.load().w2l_tune_count()), "plan_configs": bool(engine.plan_configs_enabled()), "resolved": {}}
for n in (8, 37, 128):
    G._graphs.clear()
    idx = torch.arange(n, device=dev) % 32
    r = Wav2LipRunner(G, batch_size=n)
    u8 = r.run_batch(faces[idx], mels[idx]).cpu().numpy()
    np.save(work + "/u8_%d.npy" % n, u8)
    np.save(work + "/pred_%d.npy" % n, r.last_pred_nchw().cpu().numpy())
    out["resolved"][str(n)] = [[name, fam, c, k] for name, _, fam, (c, k) in r._last.plan.resolved()]
with open(work + "/out.json", "w") as fh:
    json.dump(out, fh)
print("CHILD DONE")
'''

ONE_IN_FLIGHT = os.path.join(ROOT, "wav2lip_amd", "tune_table_one_in_flight.json")
SWITCHES = (("W2L_EXACT", "1"), ("W2L_SPLIT", "0"), ("W2L_TUNE_TABLE", ONE_IN_FLIGHT), ("W2L_TUNE_TABLE", "0"), ("W2L_PLAN_CONFIGS", "0"))
SWITCH_VARS = ("W2L_EXACT", "W2L_SPLIT", "W2L_TUNE_TABLE", "W2L_PLAN_CONFIGS", "W2L_AUTOTUNE")


def _switch_took_effect(var, value, out):
    from wav2lip_amd import _lib
    res = {int(n): [tuple(e) for e in lst] for n, lst in out["resolved"].items()}
    fams = {n: {fam for _, fam, _, _ in lst} for n, lst in res.items()}
    split_names = {_lib.FAMILY_NAMES[f] for f in _lib.SPLIT_FAMILIES}
    if (var, value) == ("W2L_EXACT", "1"):
        assert all("wino4" not in f for f in fams.values()), fams
    elif (var, value) == ("W2L_SPLIT", "0"):
        assert all(not (f & split_names) for f in fams.values()), fams
    elif var == "W2L_TUNE_TABLE" and value != "0":
        tab = pc.table_entries(value)
        assert out["tune_count"] == len(tab)
        held = 0
        for n, lst in res.items():
            for (name, key), (rec, _, c, k) in zip(pc.tune_keys(n), lst):
                assert name == rec
                if key in tab:
                    held += 1
                    assert (c, k) == tab[key], "N=%d %s resolved (%d, %d), the file holds %s" % (n, name, c, k, tab[key])
        assert held == 2 * len(pc.launches())                  # 8 and 128 are table sizes, 37 is not
        assert any("wino2s" in f for f in fams.values()), fams
    elif (var, value) == ("W2L_TUNE_TABLE", "0"):
        assert out["tune_count"] == 0
    elif (var, value) == ("W2L_PLAN_CONFIGS", "0"):
        assert [(name, c, k) for name, _, c, k in res[37]] != pc.expected_plan(64)
    if var != "W2L_PLAN_CONFIGS" and (var, value) != ("W2L_SPLIT", "0"):
        assert not out["plan_configs"]                         # these own their plans (engine.plan_configs_enabled)
    if (var, value) != ("W2L_TUNE_TABLE", "0"):
        assert out["tune_count"] > 0


def test_load_time_switches_in_fresh_processes_against_the_oracle(cuda, pool, tmp_path):
    """W2L_EXACT=1, W2L_SPLIT=0, W2L_TUNE_TABLE=<one-in-flight table>, W2L_TUNE_TABLE=0 and W2L_PLAN_CONFIGS=0 are read when the
    library loads: each runs N = 8, 37 and 128 of the pool in a fresh child process, one after another, the first failing child
    ending the test.  The parent holds every frame to the bars of this file (W2L_EXACT=1: 8 x d32, it runs no F(4x4)) and checks
    from the resolved launch lists that the switch took effect: no wino4 launch; no split-operand family; every launch the
    one-in-flight file holds resolved to the file's entry, wino2s among them; an empty table; N = 37 off the committed 64 list."""
    for var, value in SWITCHES:
        work = tmp_path / ("%s_%s" % (var, os.path.basename(value)))
        work.mkdir()
        env = {k: v for k, v in os.environ.items() if k not in SWITCH_VARS}
        env[var] = value
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(work)], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0 and "CHILD DONE" in p.stdout, "%s=%s: exit %d\n%s" % (var, value, p.returncode, p.stderr[-2000:])
        with open(str(work / "out.json")) as fh:
            out = json.load(fh)
        _switch_took_effect(var, value, out)
        tight = TIGHT_EXACT if var == "W2L_EXACT" else TIGHT
        for n in (8, 37, 128):
            y = torch.from_numpy(np.load(str(work / ("pred_%d.npy" % n))))
            u8 = np.load(str(work / ("u8_%d.npy" % n)))
            _check_frames("%s=%s N=%d" % (var, os.path.basename(value), n), pool, pc.batch_index(n), y, u8, tight)
            _check_positions(n, y, u8)
