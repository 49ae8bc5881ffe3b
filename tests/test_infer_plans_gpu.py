"""The three inference graphs (generator, SyncNet, S3FD) build the launches and compute the bytes that
tests/golden/golden_infer_plans_v1.npz records, in fp32 and in bf16 storage: launch lists with their shapes and resolved
configurations, buffer layouts, split points, scratch sizes and outputs, compared with ==.  The fixture was written by
tests/golden/make_golden_infer_plans.py on the commit before the per-precision graph classes became one class per network; outputs
are bit-reproducible across processes and boxes while W2L_AUTOTUNE is unset (wav2lip_amd/engine.py), so equality is the bar."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLDEN, "golden_infer_plans_v1.npz"))

_spec = importlib.util.spec_from_file_location("make_golden_infer_plans", os.path.join(GOLDEN, "make_golden_infer_plans.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)


def _check(prefix, out):
    """every fixture entry of one (network, precision) equals what the tree built now: the metadata key by key (a failure names
    the first launch that differs), the arrays byte for byte"""
    keys = sorted(k for k in G.files if k.startswith(prefix))
    assert keys == sorted(out) and keys
    want, got = json.loads(str(G[prefix + "meta"])), json.loads(str(out[prefix + "meta"]))
    assert sorted(want) == sorted(got)
    for k in want:
        if isinstance(want[k], list) and isinstance(got[k], list) and len(want[k]) == len(got[k]):
            for i, (w, g) in enumerate(zip(want[k], got[k])):
                assert w == g, "%s%s[%d]: %r became %r" % (prefix, k, i, w, g)
        assert want[k] == got[k], "%s%s: %r became %r" % (prefix, k, want[k], got[k])
    for k in keys:
        if not k.endswith("meta"):
            assert out[k].dtype == G[k].dtype and out[k].shape == G[k].shape and out[k].tobytes() == G[k].tobytes(), k


@pytest.fixture(scope="module", autouse=True)
def _reproducible():
    from wav2lip_amd import engine
    assert not engine.AUTOTUNE and engine.plan_configs_enabled(), "the fixture holds the table / plan_configs.json configurations"


@pytest.mark.parametrize("precision", make.PRECISIONS)
def test_generator_plan_and_frames_equal_the_fixture_through_all_three_audio_forms(cuda, precision):
    out = {}
    frames = make.generator(cuda, precision, out)
    _check("gen_%s_" % precision, out)
    want = G["gen_%s_frames" % precision]
    for form in ("windows", "starts", "rows"):
        assert frames[form].dtype == np.uint8 and frames[form].tobytes() == want.tobytes(), form
    meta = json.loads(str(out["gen_%s_meta" % precision]))
    assert len(meta["records"]) == meta["n_face"] + meta["n_audio"] + 19 and ("dispatch" in meta) == (precision == "bf16")


@pytest.mark.parametrize("precision", make.PRECISIONS)
def test_syncnet_plan_and_embeddings_equal_the_fixture_through_both_doors(cuda, precision):
    out = {}
    doors = make.syncnet(cuda, precision, out)
    _check("sync_%s_" % precision, out)
    for name, got in zip(("audio", "face"), doors["rows"]):
        assert got.dtype == np.float32 and got.tobytes() == G["sync_%s_%s" % (precision, name)].tobytes(), name


@pytest.mark.parametrize("precision", make.PRECISIONS)
def test_s3fd_ops_and_dense_tables_equal_the_fixture(cuda, precision):
    out = {}
    tables = make.s3fd(cuda, precision, out)
    _check("s3fd_%s_" % precision, out)
    assert sorted(tables) == ["dense", "rows", "rows2"] and all(len(t) == 6 for t in tables.values())
    for a, b in zip(tables["dense"], tables["rows"]):            # the address-table door at det_scale 1 gives dense_boxes' tables
        assert a.tobytes() == b.tobytes()
    assert any(float(torch.from_numpy(t)[..., 4].max()) > 0.5 for t in tables["dense"])      # and the fixture holds a detection
