"""Shared by tests/test_stream_resample_cpu.py and tests/test_stream_resample_gpu.py (streaming at a source rate of its own:
wav2lip_amd/streaming.py, w2l_resample_stream in csrc/audio_mel.hip): the rule by which an output sample is final, restated one
index at a time from oracle/resample_ref.py, the whole signal's time registers, and numpy stand-ins for the two device seams
`DeviceResampler` and `DeviceMel`.  No fixtures, no tests, nothing that needs a device."""
import numpy as np

from oracle import resample_ref

RATES = (48000, 44100, 22050, 8000, 15999, 16001)
NWIN, TABLE = 64 * 512 + 1, 512


def params(rate):
    """(ratio, index_step, K) as the issue defines them"""
    ratio = 16000.0 / rate
    index_step = int(min(1.0, ratio) * TABLE)
    return ratio, index_step, NWIN // index_step


_REGISTERS = {}


def registers(rate, n_out):
    """resample_ref.time_registers of a signal at least n_out outputs long (a prefix of a cumsum is the cumsum of the prefix)"""
    have = _REGISTERS.get(rate)
    if have is None or len(have) < n_out:
        have = _REGISTERS[rate] = resample_ref.time_registers(max(n_out, 4096), 16000.0 / rate)
        have.setflags(write=False)
    return have[:n_out]


def reads(rate, tr, total=-1):
    """(lowest, highest) source index the output with time register `tr` reads, by resample_ref.resampy_resample's own loop
    bounds; total: the signal's length when its end is known, else -1 (the right wing is not cut)"""
    ratio, index_step, _ = params(rate)
    scale = min(1.0, ratio)
    n = int(tr)
    frac = scale * (tr - n)
    offset = int(frac * TABLE)
    i_max = min(n + 1, (NWIN - offset) // index_step)
    offset = int((scale - frac) * TABLE)
    k_max = (NWIN - offset) // index_step
    if total >= 0:
        k_max = min(total - n - 1, k_max)
    return n - max(i_max, 1) + 1, n + max(k_max, 0)


def final_outputs(rate, m):
    """how many outputs of an open stream the issue's rule calls final after m source samples: n_t + K <= m - 1"""
    ratio, _, K = params(rate)
    tr = registers(rate, int(m * ratio) + 8)
    return int(np.sum(tr.astype(np.int64) + K <= m - 1))


def noise(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


class StubResampler:
    """DeviceResampler on numpy: a 16 kHz sample's "value" is its own absolute index, unwritten samples are NaN.  Checks on its
    own, for every launch, that the held source samples are the right ones and cover every index the outputs read, that an
    output is computed only when it is final, that the block-start time registers are the whole signal's, and that no 16 kHz
    sample is ever written twice."""
    instances = []

    def __init__(self, device):
        self.calls, self.buffers, self.carried = [], 0, 0
        StubResampler.instances.append(self)

    def new_buffer(self, cap16):
        self.buffers += 1
        return np.full(cap16, np.nan, np.float32)

    @staticmethod
    def buffer_bytes(buf):
        return buf.nbytes

    def compute(self, items):
        self.calls.append(sum(it[10] for it in items))
        for x, first, total, n_res, buf, buf_first, cap16, carry, rate, t0, count, tr in items:
            assert x.dtype == np.float32 and buf.shape == (cap16,) and len(tr) == count > 0
            assert (x == (np.arange(first, first + x.size) % 1000).astype(np.float32)).all()          # the right samples
            if carry is not None:
                old, old_first, c0, cn = carry
                assert old is not buf and c0 == buf_first and c0 + cn == t0
                assert not np.isnan(old[c0 - old_first:c0 - old_first + cn]).any() and np.isnan(buf[:cn]).all()
                buf[:cn] = old[c0 - old_first:c0 - old_first + cn]
                self.carried += cn
            whole = registers(rate, t0 + count)
            assert np.array_equal(np.asarray(tr).view(np.uint64), whole[t0:].view(np.uint64)), (rate, t0)   # block starts included
            for j in range(count):
                t = t0 + j
                assert 0 <= t - buf_first < cap16 and np.isnan(buf[t - buf_first]), "a sample is written once"
                if n_res < 0 or t < n_res:
                    lo, hi = reads(rate, tr[j], total)
                    assert first <= lo and hi < first + x.size, (rate, t, lo, hi, first, x.size)
                    if total < 0:
                        assert hi <= first + x.size - 1 and int(tr[j]) + params(rate)[2] <= first + x.size - 1   # final by the rule
                buf[t - buf_first] = t


def mel_reads(col, total=-1):
    """(lowest, highest) 16 kHz sample spectrogram column `col` reads, pre-emphasis predecessor included"""
    j = col * 200 + np.arange(800) - 400
    j = np.where(j < 0, -j, j)
    if total >= 0:
        j = np.where(j >= total, 2 * (total - 1) - j, j)
    return max(0, int(j.min()) - 1), int(j.max())


class StubMel:
    """DeviceMel on numpy for streams whose samples are `streaming.Resident` in a StubResampler buffer: a column's "spectrogram"
    is its own absolute number; checks that the samples a column reads are there (written, at the right place) and that nothing
    is staged for them"""
    instances = []

    def __init__(self, device):
        self.calls, self.windows = [], 0
        StubMel.instances.append(self)

    def new_window(self, cap):
        self.windows += 1
        return np.full((80, cap), np.nan, np.float32)

    def carry(self, new, old, first, count):
        assert count <= 16 and not np.isnan(old[:, first:first + count]).any()
        new[:, :count] = old[:, first:first + count]

    @staticmethod
    def window_bytes(window):
        return window.nbytes

    def compute(self, items):
        from wav2lip_amd import streaming
        self.calls.append(sum(it[7] for it in items))
        for x, first, total, window, cap, col0, lo, count in items:
            if isinstance(x, streaming.Resident):
                held = x.buffer[x.offset:x.offset + x.size]
                want = np.arange(first, first + x.size, dtype=np.float32)
            else:
                held, want = x, (np.arange(first, first + x.size) % 1000).astype(np.float32)
            for col in range(lo, lo + count):
                a, b = mel_reads(col, total)
                assert first <= a and b < first + x.size, (col, total, first, x.size)
                assert (held[a - first:b + 1 - first] == want[a - first:b + 1 - first]).all()
                assert 0 <= col - col0 < cap and np.isnan(window[:, col - col0]).all(), "a column is written once"
                window[:, col - col0] = col
