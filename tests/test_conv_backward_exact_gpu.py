"""How the training backward pass uses the forward conv kernels, held to EQUALITY with the machinery of test_conv_exact_gpu.py (integer
operands, float64 torch references, NaN guard bands, "assert the kernel that ran"; cases and bounds: tests/_conv_cases.py).

DATA GRADIENT.  autograd.dgrad_geom turns a layer into the other interpretation of its weight tensor; _conv_cases.dgrad_of restates
that (test_conv_cases_cpu.py holds the restatement to autograd.dgrad_geom and the float64 reference of every backward case to torch's
float64 AUTOGRAD input gradient of the forward layer, bit for bit).  Every (transposed, k, stride, pad, output padding) row of the
signature table runs in backward form on the fp32 implicit GEMM, the split-operand tiles and the bf16 implicit GEMM, at the smallest
extents with output padding 0, 1 and 2 per axis; every Winograd id runs with transposed = 1; conv_tp2 / conv_tp2s / tp2b run as the
gradient of a 3x3 s2 p1 conv; box64 runs with transposed = 1.

IN PLACE.  Node._data_grad accumulates with res == y.  res = 3 pre-loads the output slice with a prior gradient (integers in [-3, 3],
pad channels zero) and passes the same pointer as the residual: the slice must come back as prior + reference, guards and neighbour
channels untouched, twice with identical bits (each run starts from the same prior).
FINDING: conv_tp2 (id 10) and conv_tp2s (id 20) have no residual operand, so they cannot accumulate.  That is not a defect as long as
nothing can select them for such a launch: w2l_tune_entry_applicable declines both ids for a launch with a residual, a plan that
forces either id resolves to the implicit GEMM, and so does an unforced launch (what autograd.RawConv.run issues; its autotuner only
times ids that resolve to themselves).  test_tp2_declines_what_it_cannot_run asserts all three; the same holds for an output padding
other than (1, 1) (an odd extent of the forward layer's input).

WEIGHT RE-PACK.  test_update_repacks_every_form runs, per packed weight form, sequence A (create with w0, launch == ref(w0); update
with w1, launch == ref(w1); update scale and shift only, launch == ref(w1) under the new scale and shift) and sequence B on a fresh
handle (create with w0, update with w1 BEFORE any launch, the first launch - which builds a lazy form - == ref(w1)).  ref(w0) !=
ref(w1) is asserted on the host (and in test_conv_cases_cpu.py), so a stale form cannot pass.  The bf16 handles are updated once through
w2l_convb_update and once through ONE w2l_convb_update_many call over all of them.

`python tests/test_conv_backward_exact_gpu.py` prints the selection table (on a GPU: with the kernel the launcher reports, after the
bar; a forced bf16 split-K is not reported by the launcher, as in test_conv_exact_gpu.py).  EXPERIMENTS.md holds the table of the run
this file was written against.
"""
import ctypes as C

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file runs as a script)
import _conv_cases as cc
import test_conv_exact_gpu as fx
from wav2lip_amd import _lib
from wav2lip_amd._lib import check, current_stream

pytestmark = pytest.mark.gpu


def _id(pool, c):
    return pool.replace(" ", "_") + "-" + c.describe().replace(" ", "_")


def _dgrad_params():
    out = []
    for pool in cc.BWD_POOLS:
        out += [pytest.param(c, id=_id(pool, c)) for c in cc.exact_cases(pool)]
    return out


def _force(case, cid):
    """the same launch with another forced configuration id"""
    c = case.with_seed(case.seed)
    c.force = cid
    return c


def _declines(case, device):
    """every id in case.declines refuses the launch (w2l_tune_entry_applicable), a plan that forces it runs another family, and so
    does a launch that names no id (w2l_conv_forward's own resolution: the tune table, then the heuristic)"""
    x64, w64, scale, shift, _ = cc.int_operands(case)
    for cid in case.declines + (-1,):
        if cid >= 0:
            assert not case.applicable(cid), (case, cid)
        forced = _force(case, cid)
        x, y, res = fx._buffers(forced, device)
        _run, ran = fx._launcher(forced, w64, scale, shift, device)
        fam, got, _ks, _fl = ran(x, y, res)
        assert fam not in ("tp2", "tp2s") and got not in case.declines, (case, cid, fam, got)


def run_dgrad(case, device):
    assert case.bwd and case.act == cc.ACT_NONE and case.fwd is not None, case
    (tr, _ci, _co, k, s, p, _op), H, W = case.fwd
    assert case.out_hw() == (H, W) and case.op == cc.dgrad_op(tr, k, s, p, H, W), case      # the gradient has the extent of x
    if case.declines:
        _declines(case, device)
    return fx.run_exact(case, device)


@pytest.mark.parametrize("case", _dgrad_params())
def test_dgrad_exact(case, cuda):
    """every backward candidate: equality with float64 (bf16 storage: the reference rounded once), guards and neighbour channels
    untouched with hostile input guards, two runs with identical bits, the kernel that ran asserted from the launcher"""
    run_dgrad(case, cuda)


@pytest.mark.parametrize("name", [n for n, _p, _c in cc.BWD_REGIMES])
def test_dgrad_regime(name, cuda):
    sel = {n: c for n, _p, c in cc.select(cc.BWD_REGIMES)}
    case = sel[name]
    assert case is not None, "regime %r is empty" % name
    assert cc.regime_pred(name, cc.BWD_REGIMES)(case), (name, case)
    run_dgrad(case, cuda)


def test_tp2_declines_what_it_cannot_run(cuda):
    """conv_tp2 / conv_tp2s have no residual operand and need output padding (1, 1): for an accumulating data gradient and for the
    gradient over an odd extent, applicable(), a forced plan and the unforced launch all agree on another kernel"""
    cases = [c for c in cc.exact_cases("bwd tp2") if c.declines]
    assert {c.res for c in cases} == {0, 3} and {c.op for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    both = (cc.config_id("tp2"), cc.config_id("tp2s"))
    for c in cases:
        assert c.declines == both and c.cin % 16 == 0 and c.cout % 64 == 0      # the channel rules of both kernels are met
        _declines(c, cuda)
    plain = [c for c in cc.exact_cases("bwd tp2s") if c.cin == 16 and not c.ks][0]   # the same layer, even extents, no residual
    assert plain.applicable(both[0]) and plain.applicable(both[1])


def _accuracy_cases():
    """one case per family in backward form, in place where the family can accumulate: the deepest contraction of the pool"""
    out = []
    for pool in cc.BWD_POOLS:
        cases = [c for c in cc.exact_cases(pool) if not c.ks and not c.sliced and not c.declines]
        for fam in sorted({c.family for c in cases}):
            mine = [c for c in cases if c.family == fam]
            inplace = [c for c in mine if c.res == 3]
            best = max(inplace or mine, key=lambda c: (c.cin * c.k[0] * c.k[1], c.macs()))
            out.append(pytest.param(best, id=pool.replace(" ", "_") + "-" + fam))
    return out


@pytest.mark.parametrize("case", _accuracy_cases())
def test_dgrad_accuracy(case, cuda):
    """Gaussian operands (and a Gaussian prior gradient) in backward form against float64: 1e-4 + 1e-4 |ref| (fp32), |ref| / 128 +
    2e-5 S (bf16), the forward suite's bounds"""
    assert case.res == 3 or case.family in ("tp2", "tp2s"), case
    fx.run_accuracy(case, cuda)


# ---------------------------------------------------------------- weight re-pack
class _Layer:
    """one update case on the device: buffers, launcher, expected results"""

    def __init__(self, case, device):
        assert not fx._FAULTED, "an earlier case ended in a HIP error: nothing more is launched"
        assert cc.eligible(case) and case.exact_bound() < cc.LIMIT, case
        self.case, self.device = case, device
        x64, w0, w1, scale, shift, scale2, shift2, res64 = cc.update_operands(case)
        refs = cc.update_refs(case)
        assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[1], refs[2]), case      # a stale form cannot pass
        _D, imap = cc.image_map(case)
        self.want = [fx._expected(case, r, imap, device) for r in refs]
        assert not torch.equal(self.want[0], self.want[1]), case                                    # ... in the storage type either
        self.x, self.y, self.res = fx._buffers(case, device)
        self.x.load(x64, imap)
        if case.res == 1:
            self.res.load(res64, imap)
        self.run, self.ran = fx._launcher(case, w0, scale, shift, device)
        self.w1 = w1.float().contiguous().to(device)
        self.affine2 = (scale2.float().contiguous().to(device), shift2.float().contiguous().to(device))

    def assert_ran(self):
        fx._assert_ran(self.case, self.ran(self.x, self.y, self.res))

    def launch_equals(self, i, what):
        self.y.reset()
        self.run(self.x, self.y, self.res)
        fx._sync()
        fx._compare(self.case, self.y, self.want[i], "%r: %s" % (self.case, what))

    def update_weights(self):
        if self.case.path == "f32":
            check(_lib.load().w2l_conv_update(self.run.handle, _lib.ptr(self.w1), None, None, current_stream()), "conv_update")
        else:
            self.run.layer.update(self.w1)

    def update_affine(self):
        """scale and shift only (fp32: weight = NULL; a bf16 launch takes them per call)"""
        sc, sh = self.affine2
        if self.case.path == "f32":
            check(_lib.load().w2l_conv_update(self.run.handle, None, _lib.ptr(sc), _lib.ptr(sh), current_stream()), "conv_update")
        else:
            self.run.aff["sc"], self.run.aff["sh"] = sc, sh


def _update_params():
    return [pytest.param(c, id=c.path + "-" + c.family + "-" + c.describe().replace(" ", "_")) for c in cc.exact_cases("update")]


@pytest.mark.parametrize("case", _update_params())
def test_update_repacks_every_form(case, cuda):
    # sequence A: launch, update, launch, update scale and shift only, launch
    a = _Layer(case, cuda)
    a.assert_ran()
    a.launch_equals(0, "created with w0")
    a.update_weights()
    a.launch_equals(1, "after an update with w1 (stale packed form?)")
    a.update_affine()
    a.launch_equals(2, "after an update of scale and shift only")
    del a
    # sequence B: update before the first launch, which builds whatever form is lazy
    b = _Layer(case, cuda)
    b.update_weights()
    b.assert_ran()
    b.launch_equals(1, "updated with w1 before the first launch")


def test_update_many_repacks_every_bf16_form(cuda):
    """ONE w2l_convb_update_many call over a handle of every bf16 family (sequence A and, on fresh handles, sequence B)"""
    cases = [c for c in cc.exact_cases("update") if c.path == "bf16"]
    assert {c.family for c in cases} == {"igemm", "stem", "box64", "tp2b", "k3s_head"}
    assert {c.convb_resolve()[0] for c in cases if c.family == "stem"} == {"stem1", "stem2", "stem3"}
    lib = _lib.load()

    def update_many(layers):
        n = len(layers)
        handles = (C.c_void_p * n)(*[l.run.layer.handle.value for l in layers])
        weights = (C.c_void_p * n)(*[l.w1.data_ptr() for l in layers])
        check(lib.w2l_convb_update_many(n, handles, weights, current_stream()), "convb_update_many")
    layers = [_Layer(c, cuda) for c in cases]
    for l in layers:
        l.assert_ran()
        l.launch_equals(0, "created with w0")
    update_many(layers)
    for l in layers:
        l.launch_equals(1, "after ONE update_many call over %d layers" % len(layers))
    del layers
    fresh = [_Layer(c, cuda) for c in cases]
    update_many(fresh)
    for l in fresh:
        l.assert_ran()
        l.launch_equals(1, "update_many before the first launch")


def main():
    ran = None
    if torch.cuda.is_available():
        dev, ran = torch.device("cuda:0"), {}
        for name, _pool, case in cc.select(cc.BWD_REGIMES):
            if case is not None:
                fam, cid, ks, _fl = run_dgrad(case, dev)
                ran[name] = "%s%s%s" % (fam, " %d" % cid if cid >= 0 else "", " ks %d" % ks if ks > 1 else "")
                if case.path == "bf16" and case.ks:      # not reported by the launcher: the test's restatement of its K-steps
                    ran[name] += " (forced split-K %d: %d splits by the test's own model, unchecked)" % (case.ks, case.splits()[0])
    print(cc.table(ran, cc.BWD_REGIMES))
    for c in cc.exact_cases("update"):
        print("  update: %r" % (c,))


if __name__ == "__main__":
    main()
