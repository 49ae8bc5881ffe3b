"""Record what the bf16-storage conv launcher resolves to (tests/golden/golden_convb_resolve_v1.npz), from the launcher itself:
ConvB.resolve (the launcher's dry run behind a layer handle) for the kernel family, tile and split-K, and a plan of one
w2l_plan_add_convb item with w2l_plan_executed_flops for the executed FLOPs.  Needs a HIP device (a layer handle holds device
weights); launches nothing.  tests/test_convb_resolve_cpu.py holds the cases and checks w2l_convb_resolve_geom against the file.

    python tests/golden/make_golden_convb_resolve.py [out.npz]

row_case [R, 3]       (signature index, 0 forward / 1 data gradient, 0 / 1 residual)
row_family [R]        "igemm" | "stem<k>" | "box64" | "tp2b"            as ConvB.resolve names them
row_n_tile_ks [R, 3]  (first N, tile, ksplit): one row at every N in 1..640 where the answer changes
flop_geom [K, 12], flop_nhw_res [K, 6] = (N, H, W, residual, tile, ksplit), flop_family [K], flop_flops [K]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_convb_resolve_cpu as T                       # noqa: E402
from test_conv_gpu import SIGS                           # noqa: E402
from wav2lip_amd import bf16, engine                     # noqa: E402
from wav2lip_amd._lib import ACT_NONE, ACT_RELU, ConvGeom  # noqa: E402


def make_layer(g, dev):
    shape = (g.cin, g.cout, g.kh, g.kw) if g.transposed else (g.cout, g.cin, g.kh, g.kw)
    return bf16.ConvB(g, torch.zeros(shape, device=dev))


def plan_flops(layer, N, H, W, res, dev):
    Ho, Wo = layer.out_hw(H, W)
    x = bf16.ActB(bf16.new_buf(N, H, W, layer.cin, dev), 0, layer.cin)
    y = bf16.ActB(bf16.new_buf(N, Ho, Wo, layer.cout, dev), 0, layer.cout)
    plan = engine.Plan()
    plan.add_convb("case", layer, x, y, y if res else None)
    (_, fl), = plan.executed_flops()
    return fl


def main(out):
    dev = torch.device("cuda:0")
    row_case, row_family, row_ntk = [], [], []
    for idx in range(len(SIGS)):
        for dgrad in (0, 1):
            g, H, W = T.sig_geom(idx, dgrad)
            layer = make_layer(g, dev)
            for res in (0, 1):
                for N, fam, tile, ks in T.boundaries(lambda N: layer.resolve(N, H, W, bool(res))):
                    row_case.append((idx, dgrad, res))
                    row_family.append(fam)
                    row_ntk.append((N, tile, ks))

    cases = [T.sig_geom(idx, 0) + (3, SIGS[idx][8]) for idx in range(len(SIGS))]
    cases = [(g, N, H, W, res) for g, H, W, N, res in cases]
    cases.append((ConvGeom(0, 64, 64, 3, 3, 1, 1, 1, 1, 0, 0, ACT_RELU), 342, 48, 32, 1))        # box64
    cases.append((ConvGeom(0, 6, 16, 7, 7, 1, 1, 3, 3, 0, 0, ACT_RELU), 30, 96, 96, 0))          # stem
    cases.append((ConvGeom(1, 64, 32, 3, 3, 2, 2, 1, 1, 1, 1, ACT_NONE), 128, 16, 32, 0))        # tp2b: thin_64_32
    for idx in (20, 21, 22, 23, 25, 42):                                                         # test_split_k's layers at its N
        g, H, W = T.sig_geom(idx, 0)
        cases.append((g, 5, H, W, SIGS[idx][8]))
    i256 = next(i for i, s in enumerate(SIGS) if s[:8] == ("c", 3, 1, 1, 256, 256, 24, 24))
    g256, H, W = T.sig_geom(i256, 0)                      # 256 -> 256 at 24x24: the 256x256 tile from its first N on
    layer = make_layer(g256, dev)
    n256 = next(N for N in range(1, T.N_MAX + 1) if layer.resolve(N, H, W, True)[:2] == ("igemm", 5))
    cases.append((g256, n256, H, W, 1))

    flop_geom, flop_shape, flop_family, flop_flops = [], [], [], []
    for g, N, H, W, res in cases:
        layer = make_layer(g, dev)
        fam, tile, ks = layer.resolve(N, H, W, bool(res))
        flop_geom.append(T.geom_tuple(g))
        flop_shape.append((N, H, W, int(res), tile, ks))
        flop_family.append(fam)
        flop_flops.append(plan_flops(layer, N, H, W, bool(res), dev))
    assert any(f == "igemm" and s[5] > 1 for f, s in zip(flop_family, flop_shape))
    assert {"box64", "tp2b", "stem1"} <= set(flop_family)

    np.savez_compressed(out, row_case=np.array(row_case, np.int32), row_family=np.array(row_family),
                        row_n_tile_ks=np.array(row_ntk, np.int32), flop_geom=np.array(flop_geom, np.int32),
                        flop_nhw_res=np.array(flop_shape, np.int32), flop_family=np.array(flop_family),
                        flop_flops=np.array(flop_flops, np.int64))
    print("%d boundary rows over %d cases, %d FLOP cases, families %s -> %s"
          % (len(row_case), len(SIGS) * 4, len(cases), sorted(set(row_family) | set(flop_family)), out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden_convb_resolve_v1.npz"))
