"""The opt-in bf16 path of SyncNet scoring without a device: the `--precision` flag of `python -m wav2lip_amd.calculate_scores`,
the precision check of `evaluation.lse_like` / `lse_many`, the 2 GiB buffer rule of the bf16 plan as a function of the batch
size, and the convb kernel every SyncNet layer resolves to at the batch sizes the GPU tests run."""
import pytest
import torch

from wav2lip_amd import bf16
from wav2lip_amd._lib import ACT_RELU, ConvGeom


def test_cli_parser_takes_precision_and_the_reference_parser_does_not():
    from wav2lip_amd import calculate_scores as cs, inference
    base = ["--data_root", "d", "--checkpoint_path", "c"]
    assert cs.cli_parser.parse_args(base).precision == "fp32"
    a = cs.cli_parser.parse_args(base + ["--precision", "bf16"])
    assert a.precision == "bf16" and inference.CLI_PRECISION[a.precision] == "bf16" and a.face_det_precision == "fp32"
    with pytest.raises(SystemExit):
        cs.cli_parser.parse_args(base + ["--precision", "fp16"])
    assert "SyncNet arithmetic" in cs.build_cli_parser().format_help()
    with pytest.raises(SystemExit):                                    # build_parser holds the reference's flags only
        cs.build_parser().parse_args(base + ["--precision", "bf16"])
    assert not hasattr(cs.parser.parse_args(base), "precision")


class _Untouchable:
    """a model that fails the test as soon as anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("the model was touched (%s) before the precision was checked" % name)


def test_precision_is_checked_before_any_device_work():
    from wav2lip_amd import evaluation
    with pytest.raises(ValueError, match="precision"):
        evaluation.lse_many(_Untouchable(), [], precision="half")
    with pytest.raises(ValueError, match="precision"):
        evaluation.lse_like(_Untouchable(), None, None, precision="half")
    with pytest.raises(ValueError, match="precision"):
        evaluation.lse_many(_Untouchable(), [], precision="fp32")        # the API's names are "f32" / "bf16"


def test_bf16_buffer_rule_is_a_function_of_the_batch_size():
    """the largest buffer is the stem's 48 x 96 x 32 bf16 output, 294 912 bytes per window: the first batch that reaches 2 GiB is
    ceil(2**31 / 294912) = 7282"""
    from wav2lip_amd.models import syncnet
    one = syncnet.bf16_buffer_sizes(1)
    assert max(one) == 48 * 96 * 32 * 2 == 294912 and one[0] == 48 * 96 * 16 * 2 and one[1] == 80 * 16 * 8 * 2
    assert len(one) == 2 + len(syncnet.SYNC_FACE_ENCODER) + len(syncnet.audio_encoder_rows(2))
    assert one[2 + len(syncnet.SYNC_FACE_ENCODER) - 1] == one[-1] == 512 * 2                  # both encoders end at 1 x 1 x 512
    assert syncnet.bf16_buffer_sizes(128) == [128 * b for b in one]
    first = syncnet.bf16_batch_limit()
    assert first == -(-(1 << 31) // 294912) == 7282
    assert max(syncnet.bf16_buffer_sizes(first)) >= 1 << 31 > max(syncnet.bf16_buffer_sizes(first - 1))
    syncnet.check_bf16_buffers(first - 1)
    with pytest.raises(RuntimeError, match=r"batch of %d windows" % first):
        syncnet.check_bf16_buffers(first)
    with pytest.raises(RuntimeError, match="2 GiB"):                   # the graph checks before it allocates: no device is needed
        syncnet._SyncGraph(None, first, 48, 96, torch.device("cpu"), precision="bf16")


def _layers():
    """(name, ConvGeom, H, W, residual) of every SyncNet layer, from the model's own tables"""
    from wav2lip_amd import engine
    from wav2lip_amd.models import syncnet
    out = []
    for name, rows, (h, w) in (("face_encoder", syncnet.SYNC_FACE_ENCODER, (48, 96)),
                               ("audio_encoder", syncnet.audio_encoder_rows(2), (80, 16))):
        for j, (kind, cin, cout, k, s, p, _) in enumerate(rows):
            sh, sw = engine._pair(s)
            out.append(("%s.%d" % (name, j), ConvGeom(0, cin, cout, k, k, sh, sw, p, p, 0, 0, ACT_RELU), h, w, kind == "r"))
            h, w = (h + 2 * p - k) // sh + 1, (w + 2 * p - k) // sw + 1
        assert (h, w) == (1, 1), name
    return out


@pytest.mark.parametrize("N", [1, 7, 8, 128])
def test_every_syncnet_layer_resolves_to_a_convb_kernel(N):
    layers = _layers()
    assert len(layers) == 17 + 14 and sum(r for *_, r in layers) == 9 + 8
    got = []
    for name, g, h, w, res in layers:
        fam, tile, ks = bf16.ConvB.resolve_geom(g, N, h, w, res)          # raises on a geometry the launcher refuses
        assert fam in ("igemm", "box64", "tp2b") or fam.startswith("stem"), (name, fam)
        assert ks >= 1
        got.append((name, fam, tile, ks))
    print("N=%d: %s" % (N, [(f, t, k) for _, f, t, k in got]))
    assert got[0][1].startswith("stem") or got[0][1] == "igemm"
