"""w2l_color_match_u8 (csrc/color_match.hip) against the numpy model of tests/_color_cases.py, byte for byte.  Prediction,
reference and output are carved from larger buffers at base offsets 0 and 1; the bytes around the output, the reference and (out
of place) the prediction must come back unchanged, and whole buffers are compared.  Every refused call gets buffers that would
hold the size it names, so that nothing could be written out of bounds even if the check were missing."""
import functools

import numpy as np
import pytest
import torch

import _color_cases as CC

pytestmark = pytest.mark.gpu
GUARD = 16
MODES = sorted(CC.MODES)


def _lib3():
    from wav2lip_amd import _lib
    return _lib.load(), _lib.current_stream(), _lib.ptr


@functools.lru_cache(maxsize=None)
def _group(S, mode):
    """(pred, ref, the model's output) of the case group of size S: computed once, shared, read-only"""
    group = dict(CC.case_groups())[S]
    pred, ref = CC.stack(group)
    want = CC.model_rows(pred, ref, mode)
    for a in (pred, ref, want):
        a.setflags(write=False)
    return pred, ref, want


def _carve(data, off, cuda, seed):
    """a device buffer of noise with `data` at byte GUARD + off (torch's allocations are 256-byte aligned); (host copy, device,
    lo, hi)"""
    host = np.random.default_rng(seed).integers(0, 256, GUARD + off + data.size + GUARD, dtype=np.uint8)
    lo, hi = GUARD + off, GUARD + off + data.size
    host[lo:hi] = data.reshape(-1)
    dev = torch.from_numpy(host.copy()).to(cuda)
    assert dev.data_ptr() % 16 == 0
    return host, dev, lo, hi


def _launch(cuda, pred, ref, S, mode, in_place=False, offs=(0, 0, 0), B=None):
    """one launch over B rows; returns the output rows.  Checks the guards of the output, the reference and the prediction."""
    lib, s, ptr = _lib3()
    B = len(pred) if B is None else B
    ph, pd, plo, phi = _carve(pred, offs[0], cuda, 91)
    rh, rd, rlo, rhi = _carve(ref, offs[1], cuda, 92)
    if in_place:
        oh, od, olo, ohi = ph, pd, plo, phi
    else:
        oh, od, olo, ohi = _carve(np.full(pred.shape, 0xA5, np.uint8), offs[2], cuda, 93)
    rc = lib.w2l_color_match_u8(s, B, ptr(pd[plo:phi]), ptr(rd[rlo:rhi]), S, CC.MODES[mode], ptr(od[olo:ohi]))
    assert rc == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    got = od.cpu().numpy()
    assert np.array_equal(got[:olo], oh[:olo]) and np.array_equal(got[ohi:], oh[ohi:]), "bytes around the output changed"
    assert np.array_equal(rd.cpu().numpy(), rh), "the reference was written"
    if not in_place:
        assert np.array_equal(pd.cpu().numpy(), ph), "the prediction was written"
    return got[olo:ohi].reshape(pred.shape)


def _diff(case, got, want):
    bad = np.argwhere(got != want)
    return "%s: %d bytes differ, first at %s: got %d, want %d" % (case, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [96, 6, 2, 256])
def test_the_case_list_in_one_launch(cuda, S, mode):
    """every case of a size side by side in ONE launch: flat prediction, flat reference, gains clamped and exactly on 128 and 512,
    saturation at both ends, three gains in one row, identity, noise; S = 256 holds the largest sums and numerators"""
    pred, ref, want = _group(S, mode)
    assert len(pred) >= 2
    got = _launch(cuda, pred, ref, S, mode)
    names = list(dict(CC.case_groups())[S])
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), _diff("S %d %s case %s" % (S, mode, name), got[k], want[k])
    assert not np.array_equal(got, pred)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("S", [96, 6])
def test_rows_at_base_offsets_0_and_1(cuda, S, B, mode, in_place):
    """B rows with prediction, reference and output at every combination of base offsets 0 and 1 (dword and byte paths of each
    pointer on its own); in place the output IS the prediction"""
    pred, ref, want = _group(S, mode)
    pred, ref, want = pred[2:2 + B], ref[2:2 + B], want[2:2 + B]
    assert len(pred) == B
    for po in (0, 1):
        for ro in (0, 1):
            for oo in ((po,) if in_place else (0, 1)):
                got = _launch(cuda, pred, ref, S, mode, in_place=in_place, offs=(po, ro, oo))
                assert np.array_equal(got, want), _diff("S %d B %d %s offsets %s" % (S, B, mode, (po, ro, oo)), got, want)


def test_in_place_equals_out_of_place_on_the_product_size(cuda):
    pred, ref, want = _group(96, "full")
    a = _launch(cuda, pred, ref, 96, "full")
    b = _launch(cuda, pred, ref, 96, "full", in_place=True)
    assert np.array_equal(a, b) and np.array_equal(a, want)


def test_a_launch_names_only_its_b_rows(cuda):
    """B = 3 of 5 rows: rows 3 and 4 of the output buffer keep their fill"""
    pred, ref, want = _group(6, "full")
    pred, ref, want = pred[:5], ref[:5], want[:5]
    got = _launch(cuda, pred, ref, 6, "full", B=3)
    assert np.array_equal(got[:3], want[:3]) and (got[3:] == 0xA5).all()


def test_b_0_writes_nothing(cuda):
    lib, s, ptr = _lib3()
    pred, ref, _ = _group(6, "mean")
    got = _launch(cuda, pred, ref, 6, "mean", B=0)
    assert (got == 0xA5).all()
    assert lib.w2l_color_match_u8(s, 0, None, None, 96, 1, None) == 0           # no pointer is looked at when B == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("what,B,S,mode,null", [("odd S", 1, 95, 1, None), ("S above 256", 1, 258, 2, None), ("S of 0", 1, 0, 1, None),
                                                ("negative S", 1, -96, 1, None), ("mode 0", 1, 96, 0, None), ("mode 3", 1, 96, 3, None),
                                                ("negative B", -1, 96, 1, None), ("NULL pred", 1, 96, 1, 0), ("NULL ref", 1, 96, 2, 1),
                                                ("NULL out", 1, 96, 2, 2)],
                         ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_bad_arguments_are_refused_with_a_message_and_nothing_is_written(cuda, what, B, S, mode, null):
    lib, s, ptr = _lib3()
    n = 258 * 258 * 3                                                           # holds the largest size a refused call names
    pred = torch.full((n,), 0x11, dtype=torch.uint8, device=cuda)
    ref = torch.full((n,), 0x22, dtype=torch.uint8, device=cuda)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    args = [ptr(pred), ptr(ref), ptr(out)]
    if null is not None:
        args[null] = None
    rc = lib.w2l_color_match_u8(s, B, args[0], args[1], S, mode, args[2])
    msg = lib.w2l_last_error()
    torch.cuda.synchronize()
    assert rc != 0, what
    assert msg and b"color_match" in msg, (what, msg)
    assert bool((out == 0xA5).all()) and bool((pred == 0x11).all()) and bool((ref == 0x22).all()), what
