"""JPEG encoding of face crops on the device (w2l_jpeg_encode_rows, csrc/jpeg.hip): the crops of a detector batch are encoded
where they lie, inside the frames the detector has just read, and only the finished files' bytes come back to the host.  The
files are byte-equal to what the host path of `preprocess` writes (PIL / libjpeg-turbo at the same quality, 4:2:0, standard
Huffman tables): baseline JPEG is integer arithmetic end to end.

    encode_crops(frames, boxes, quality=95)      -> list[bytes], one complete JFIF file per box
    CropEncoder(...).submit(frames, boxes, paths); .collect(); .finish()     the asynchronous form `preprocess --jpeg device` uses

Per batch: the row table (w2l_frame_row) and the slots' capacities are staged in ONE pinned buffer and copied in once, two kernels
run whatever the batch size is (on the current stream; CropEncoder's worker thread has a stream of its own), and two copies come
back: the lengths, then the used part of the slots.  There is no host fallback: a CPU tensor or a missing library raises
RuntimeError.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor, wait

import numpy as np

from . import _lib

HEADER_BYTES = 623                # SOI .. SOS; height at offset 163, width at 165 (big-endian 16-bit each)
MAX_BLOCK_BYTES = 2 * 208         # a block codes at most 22 bits of DC + 63 x 26 bits of AC = 208 bytes; stuffing can double them
MAX_ROWS = 65535                  # rows of one w2l_jpeg_encode_rows launch
MAX_BLOCKS = 1 << 20              # blocks of one crop
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def blocks(h, w):
    """8x8 blocks of an h x w crop at 4:2:0: six per 16x16 MCU"""
    return 6 * (-(-int(h) // 16)) * (-(-int(w) // 16))


def capacity(h, w):
    """bytes no file of an h x w crop can exceed: 625 (header + EOI) + 416 per block.  Slots of this size make the kernel's
    `lengths[b] = -1` (the file did not fit) a guard that never fires."""
    return HEADER_BYTES + 2 + MAX_BLOCK_BYTES * blocks(h, w)


def header(h, w, quality):
    """the 623 bytes in front of the entropy stream of an h x w file at `quality` (built by the library, which also hands them
    to the kernel)"""
    buf = (C.c_uint8 * HEADER_BYTES)()
    _lib.check(_lib.load().w2l_jpeg_header(int(h), int(w), int(quality), buf), "jpeg_header")
    return bytes(buf)


def quant_tables(quality):
    """(luma, chroma) quantisers at `quality`, uint8 [64] each in natural (row-major) order, as the header carries them"""
    hd = np.frombuffer(header(1, 1, quality), dtype=np.uint8)
    out = []
    for off in (25, 94):                          # the two DQT payloads, zigzag order
        t = np.empty(64, dtype=np.uint8)
        t[list(ZIGZAG)] = hd[off:off + 64]
        out.append(t)
    return tuple(out)


def _frame_list(frames):
    """[(tensor keeping the memory alive, device address, H, W)] of a [N,H,W,3] tensor, a [H,W,3] tensor or a list of either"""
    import torch
    out = []
    for t in (frames if isinstance(frames, (list, tuple)) else [frames]):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("jpeg: frames must be device tensors (there is no host fallback), got %s"
                               % (t.device if isinstance(t, torch.Tensor) else type(t).__name__))
        if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3 or not t.is_contiguous():
            raise ValueError("jpeg: frames must be contiguous uint8 [N,H,W,3] or [H,W,3] BGR, got %s %s" % (t.dtype, tuple(t.shape)))
        H, W = int(t.shape[-3]), int(t.shape[-2])
        for i in range(t.shape[0] if t.dim() == 4 else 1):
            out.append((t, t.data_ptr() + i * H * W * 3, H, W))
    return out


class _Plan:
    """a validated batch: the row table and the capacities as host arrays, made without touching the device"""

    def __init__(self, frames, boxes, quality, frame_index):
        from .multiclip import FRAME_ROW
        fl = _frame_list(frames)
        n = len(boxes)
        if n < 1 or n > MAX_ROWS:
            raise ValueError("jpeg: %d crops in one batch (1 .. %d)" % (n, MAX_ROWS))
        if not 1 <= int(quality) <= 100:
            raise ValueError("jpeg: quality %r is outside [1, 100]" % (quality,))
        idx = np.arange(n) if frame_index is None else np.asarray([int(i) for i in frame_index], dtype=np.int64)
        if len(idx) != n or (idx < 0).any() or (idx >= len(fl)).any():
            raise ValueError("jpeg: %d boxes, %d frames, frame_index %r" % (n, len(fl), frame_index))
        if any(f[0].device != fl[0][0].device for f in fl):
            raise ValueError("jpeg: the frames of one batch lie on one device")
        b = np.asarray([[int(v) for v in box] for box in boxes], dtype=np.int64).reshape(n, 4)
        x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        H = np.asarray([f[2] for f in fl], dtype=np.int64)[idx]
        W = np.asarray([f[3] for f in fl], dtype=np.int64)[idx]
        bad = ~((0 <= y1) & (y1 < y2) & (y2 <= H) & (0 <= x1) & (x1 < x2) & (x2 <= W) & (y2 - y1 <= 65535) & (x2 - x1 <= 65535))
        if bad.any():
            r = int(np.argmax(bad))
            raise ValueError("face box (x1=%d, y1=%d, x2=%d, y2=%d) is empty, outside the %dx%d frame or larger than a JPEG can be"
                             % (x1[r], y1[r], x2[r], y2[r], H[r], W[r]))
        self.max_blocks = int((6 * (-(-(y2 - y1) // 16)) * (-(-(x2 - x1) // 16))).max())
        if self.max_blocks > MAX_BLOCKS:
            raise ValueError("jpeg: a crop of %d blocks (at most %d)" % (self.max_blocks, MAX_BLOCKS))
        # every slot holds the largest crop's bound, so that the used part of all slots comes back as one strided copy
        self.stride = -(-(HEADER_BYTES + 2 + MAX_BLOCK_BYTES * self.max_blocks) // 16) * 16
        self.table = np.zeros(n, FRAME_ROW)
        self.table["src"] = np.asarray([f[1] for f in fl], dtype=np.uint64)[idx]
        self.table["H"], self.table["W"] = H, W
        self.table["y1"], self.table["y2"], self.table["x1"], self.table["x2"] = y1, y2, x1, x2
        self.n, self.quality, self.device, self.keep = n, int(quality), fl[0][0].device, [f[0] for f in fl]

    def run(self):
        """table and capacities in one pinned buffer and one copy in, two kernels on the current stream, the lengths back, then
        the used part of the slots: the files' bytes"""
        import torch
        lib = _lib.load()
        n, stride = self.n, self.stride
        nb = -(-self.table.nbytes // 16) * 16
        with torch.cuda.device(self.device):
            out = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
            host = torch.empty(nb + 4 * n, dtype=torch.uint8, pin_memory=True)          # the table, then cap[n]
            self.table["dst"] = out.data_ptr() + np.arange(n, dtype=np.int64) * stride
            host.numpy()[:self.table.nbytes] = self.table.view(np.uint8)
            host.numpy()[nb:].view(np.int32)[:] = stride
            staged = host.to(self.device, non_blocking=True)                             # one copy in
            ws_bytes = int(lib.w2l_jpeg_workspace_bytes(n, self.max_blocks))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            lengths_dev = torch.empty(n, dtype=torch.int32, device=self.device)
            _lib.check(lib.w2l_jpeg_encode_rows(_lib.current_stream(), n, _lib.ptr(staged), C.c_void_p(staged.data_ptr() + nb),
                                                self.quality, self.max_blocks, _lib.ptr(lengths_dev), _lib.ptr(ws), ws_bytes),
                       "jpeg_encode_rows")
            lengths = lengths_dev.cpu().numpy().astype(np.int64)                         # the first copy back (waits for the kernels)
            if (lengths < HEADER_BYTES + 2).any() or (lengths > stride).any():
                raise RuntimeError("jpeg: the device encoder refused a crop (lengths %s at capacity %d)" % (lengths.tolist(), stride))
            data = out.view(n, stride)[:, :int(lengths.max())].cpu().numpy()            # the second and last
        self.keep = None
        return [data[i, :lengths[i]].tobytes() for i in range(n)]


def encode_crops(frames, boxes, quality=95, frame_index=None):
    """The JFIF files of `frames[frame_index[i]][y1:y2, x1:x2]` for boxes[i] = (x1, y1, x2, y2) (the order
    FaceAlignment.get_detections_for_batch returns), as a list of bytes.  `frames`: a device uint8 tensor [N,H,W,3] BGR, or a list
    of such tensors (or single [H,W,3] frames) of different shapes, counted through; frame_index None: crop i reads frame i.  Runs
    on the current stream; boxes are validated here (ValueError), the kernel takes them as they are."""
    return _Plan(frames, boxes, quality, frame_index).run()


def _write_file(dst, data):
    with open(dst, "wb") as fh:
        fh.write(data)


class CropEncoder:
    """The asynchronous form.  `submit(frames, boxes, paths)` validates the batch, records an event on the current stream (the
    frames are complete from there on) and returns; one worker thread with a stream of its own waits for that event, encodes the
    batch, takes the bytes off the device and hands (path, bytes) to the thread pool, whose job is the file write.  So the
    encoding, both copies back and the writes overlap the caller's next batch, on the device and on the host, as the PIL pool of
    the host path does.  `collect` waits for the oldest batch, `finish` for everything; either raises what went wrong.  At most
    `max_batches` batches are pending (their frames stay alive that long) and at most `max_files` writes wait in the pool."""

    def __init__(self, quality=95, pool=None, max_batches=2, max_files=256):
        self.quality, self.max_batches, self.max_files = int(quality), int(max_batches), int(max_files)
        self._own = pool is None
        self.pool = pool if pool is not None else ThreadPoolExecutor(4)
        self._worker = ThreadPoolExecutor(1)          # one thread: batches keep their order and share one side stream
        self._stream = None
        self.jobs, self.writes = [], []

    def submit(self, frames, boxes, paths, frame_index=None):
        import torch
        paths = list(paths)
        if len(paths) != len(boxes):
            raise ValueError("CropEncoder: %d paths for %d boxes" % (len(paths), len(boxes)))
        plan = _Plan(frames, boxes, self.quality, frame_index)
        with torch.cuda.device(plan.device):
            ready = torch.cuda.Event()
            ready.record()
        self.jobs.append(self._worker.submit(self._encode, plan, paths, ready))
        while len(self.jobs) > self.max_batches:
            self.collect()

    def _encode(self, plan, paths, ready):
        import torch
        with torch.cuda.device(plan.device):
            if self._stream is None or self._stream.device != plan.device:
                self._stream = torch.cuda.Stream(plan.device)
            with torch.cuda.stream(self._stream):
                self._stream.wait_event(ready)
                data = plan.run()
        return [self.pool.submit(_write_file, p, d) for p, d in zip(paths, data)]

    def collect(self):
        """wait for the oldest pending batch (its writes are then in the pool); False when nothing was pending"""
        if not self.jobs:
            return False
        self.writes += self.jobs.pop(0).result()
        while len(self.writes) > self.max_files:
            self.writes.pop(0).result()
        return True

    def drain(self):
        """wait for everything pending without raising (an error path's clean-up); the errors stay with `finish`"""
        wait(self.jobs)
        for j in self.jobs:
            if j.exception() is None:
                self.writes += j.result()
        self.jobs = []
        wait(self.writes)
        self.writes = []

    def finish(self):
        """every submitted file is on disk when this returns"""
        try:
            while self.collect():
                pass
            for f in self.writes:
                f.result()
        finally:
            self.drain()

    def close(self):
        """`finish`, then the end of the threads this encoder made itself"""
        try:
            self.finish()
        finally:
            self._worker.shutdown()
            if self._own:
                self.pool.shutdown()


