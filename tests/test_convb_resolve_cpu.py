"""w2l_convb_resolve_geom - the bf16-storage launcher's shape rules without a layer handle or a device - against the answers
recorded from the launcher itself (tests/golden/make_golden_convb_resolve.py: ConvB.resolve and w2l_plan_executed_flops on the
GPU, before the rules moved into one function).  Exact: every dispatch boundary of the 58 hot-path signatures, forward and data
gradient, with and without a residual, over N = 1..640, and the executed FLOPs of every kernel family.  Needs no GPU."""
import os

import numpy as np

from conftest import ROOT
from test_conv_gpu import SIGS
from wav2lip_amd import autograd, bf16
from wav2lip_amd._lib import ACT_LEAKY, ACT_RELU, ConvGeom

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_convb_resolve_v1.npz")
N_MAX = 640
GEOM_FIELDS = ("transposed", "cin", "cout", "kh", "kw", "sh", "sw", "ph", "pw", "oph", "opw", "act")


def _pair(v):
    return tuple(v) if isinstance(v, tuple) else (v, v)


def sig_geom(idx, dgrad):
    """(geometry, H, W) of signature `idx` as tests/test_bf16_conv_gpu.py launches it: forward at its own H x W, or its data
    gradient (autograd.dgrad_geom) over the forward's output extent"""
    kind, k, stride, pad, cin, cout, H, W, _, outpad = SIGS[idx]
    (kh, kw), s, p, op = _pair(k), _pair(stride), _pair(pad), _pair(outpad)
    g = ConvGeom(int(kind == "t"), cin, cout, kh, kw, s[0], s[1], p[0], p[1], op[0], op[1], ACT_LEAKY if kind == "n" else ACT_RELU)
    if not dgrad:
        return g, H, W
    Ho, Wo = autograd.out_hw(g, H, W)
    return autograd.dgrad_geom(g, H, W), Ho, Wo


def geom_tuple(g):
    return tuple(int(getattr(g, f)) for f in GEOM_FIELDS)


def boundaries(resolve):
    """[(first N, family, tile, ksplit)]: one row at every N in 1..N_MAX where resolve(N) changes"""
    rows, last = [], None
    for N in range(1, N_MAX + 1):
        r = resolve(N)
        if r != last:
            rows.append((N,) + r)
            last = r
    return rows


def test_every_dispatch_boundary_of_the_hot_path_signatures():
    gold = np.load(GOLDEN)
    assert gold["row_case"].shape[0] == gold["row_n_tile_ks"].shape[0] == gold["row_family"].shape[0]
    want = {}
    for case, fam, ntk in zip(gold["row_case"].tolist(), gold["row_family"].tolist(), gold["row_n_tile_ks"].tolist()):
        want.setdefault(tuple(case), []).append((ntk[0], fam, ntk[1], ntk[2]))
    assert len(want) == len(SIGS) * 4
    for idx in range(len(SIGS)):
        for dgrad in (0, 1):
            g, H, W = sig_geom(idx, dgrad)
            for res in (0, 1):
                got = boundaries(lambda N: bf16.ConvB.resolve_geom(g, N, H, W, bool(res)))
                assert got == want[(idx, dgrad, res)], (idx, dgrad, res, geom_tuple(g), H, W)


def test_executed_flops_of_every_family():
    gold = np.load(GOLDEN)
    geoms, shapes, flops, fams = gold["flop_geom"], gold["flop_nhw_res"], gold["flop_flops"], gold["flop_family"].tolist()
    assert len(geoms) >= len(SIGS) + 5
    assert {"igemm", "stem1", "box64", "tp2b"} <= set(fams)
    assert any(f == "igemm" and int(s[4]) == 5 for f, s in zip(fams, shapes)), "the 256x256 tile"
    assert any(f == "igemm" and int(s[5]) > 1 for f, s in zip(fams, shapes)), "a split-K launch"
    for gt, (N, H, W, res, tile, ks), fl, fam in zip(geoms.tolist(), shapes.tolist(), flops.tolist(), fams):
        g = ConvGeom(*gt)
        assert bf16.ConvB.resolve_geom(g, N, H, W, bool(res), flops=True) == (fam, tile, ks, fl), (gt, N, H, W, res)
