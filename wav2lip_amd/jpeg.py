"""JPEG encoding of face crops on the device (w2l_jpeg_encode_rows, csrc/jpeg.hip): the crops of a detector batch are encoded
where they lie, inside the frames the detector has just read, and only the finished files' bytes come back to the host.  The
files are byte-equal to what the host path of `preprocess` writes (PIL / libjpeg-turbo at the same quality, 4:2:0, standard
Huffman tables): baseline JPEG is integer arithmetic end to end.

    encode_crops(frames, boxes, quality=95)      -> list[bytes], one complete JFIF file per box
    CropEncoder(...).submit(frames, boxes, paths); .collect(); .finish()     the asynchronous form `preprocess --jpeg device` uses

Per batch: the row table (w2l_frame_row) and the slots' capacities are staged in ONE pinned buffer (staging.py) and copied in once,
two kernels run whatever the batch size is (on the current stream; CropEncoder's worker thread has a stream of its own), and two copies come
back: the lengths, then the used part of the slots.  There is no host fallback: a CPU tensor or a missing library raises
RuntimeError.

The read side (w2l_jpeg_decode_rows, csrc/jpeg_decode.hip): baseline 4:2:0 files - what `preprocess` writes in either mode, and
what cv2.imwrite wrote for the reference - are decoded on the device to the pixels PIL / libjpeg-turbo decodes, byte for byte.

    probe(data)                  -> (H, W); UnsupportedJpeg with the parser's reason for a file outside that class
    decode_files(datas, device)  -> list of device uint8 [H,W,3] BGR tensors, views of one buffer

Per batch: the files' entropy-coded segments, the row table (w2l_jpeg_row) and the de-duplicated table sets are staged in ONE
pinned buffer and copied in once, one memset and three kernels run on the current stream whatever the batch size is, and one copy
of `status` comes back.  No host fallback here either.

Motion-JPEG frames (w2l_jpeg_encode_rows_rst, w2l_jpeg_decode_rows_rst): whole frames coded with RESTART INTERVALS, so that a
frame is many independent byte-aligned streams instead of one serial one - byte-equal to PIL's `restart_marker_rows` in both
directions.  The functions above keep refusing such files; these take them and the plain class together.

    encode_frames(frames, quality=95, restart_rows=1, boxes=None)  -> list[bytes], one complete file per frame (or per box)
    parse_frame(data)                                               -> (the _lib.JpegInfo, Ri in MCUs; 0: no restart interval)
    decode_frames(datas, device)                                    -> list of device uint8 [H,W,3] BGR tensors; one lane per interval
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor, wait

import numpy as np

from . import _lib
from ._lib import FRAME_ROW, JPEG_ROW, JPEG_SEGMENT
from .staging import Staging, align

HEADER_BYTES = 623                # SOI .. SOS; height at offset 163, width at 165 (big-endian 16-bit each)
HEADER_BYTES_RST = 629            # with DRI (FF DD 00 04 Ri) at offset 609, between the last DHT and SOS
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

    def __init__(self, frames, boxes, quality, frame_index, restart_rows=None):
        fl = _frame_list(frames)
        if boxes is None:                                  # whole frames
            boxes = [(0, 0, f[3], f[2]) for f in fl]
        n = len(boxes)
        if restart_rows is not None and not 1 <= int(restart_rows) <= 65535:
            raise ValueError("jpeg: restart_rows %r is outside [1, 65535]" % (restart_rows,))
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
        self.stride = align(HEADER_BYTES + 2 + MAX_BLOCK_BYTES * self.max_blocks)
        self.restart_rows = None if restart_rows is None else int(restart_rows)
        if self.restart_rows is not None:                  # capacity_rst of the largest crop: DRI and 4 bytes per interval on top
            mw, mh = -(-(x2 - x1) // 16), -(-(y2 - y1) // 16)
            ri = np.minimum(self.restart_rows * mw, 65535)
            self.stride = align(int((HEADER_BYTES_RST + 2 + MAX_BLOCK_BYTES * 6 * mw * mh + 4 * (-(-(mw * mh) // ri))).max()))
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
        with torch.cuda.device(self.device):
            out = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
            st = Staging(self.device)
            rows, cap = st.table(FRAME_ROW, n), st.reserve(4 * n, dtype=np.int32)         # the table, then cap[n]
            st.allocate()
            st.view(rows)[:] = self.table
            st.view(rows)["dst"] = out.data_ptr() + np.arange(n, dtype=np.int64) * stride
            st.view(cap)[:] = stride
            st.upload()                                                                  # one copy in
            lengths_dev = torch.empty(n, dtype=torch.int32, device=self.device)
            if self.restart_rows is None:
                ws_bytes = int(lib.w2l_jpeg_workspace_bytes(n, self.max_blocks))
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                _lib.check(lib.w2l_jpeg_encode_rows(_lib.current_stream(), n, _lib.ptr(st.dev), C.c_void_p(st.address(cap)),
                                                    self.quality, self.max_blocks, _lib.ptr(lengths_dev), _lib.ptr(ws), ws_bytes),
                           "jpeg_encode_rows")
            else:
                ws_bytes = int(lib.w2l_jpeg_workspace_bytes_rst(n, self.max_blocks))
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                _lib.check(lib.w2l_jpeg_encode_rows_rst(_lib.current_stream(), n, _lib.ptr(st.dev), C.c_void_p(st.address(cap)),
                                                        self.quality, self.max_blocks, self.restart_rows, _lib.ptr(lengths_dev),
                                                        _lib.ptr(ws), ws_bytes), "jpeg_encode_rows_rst")
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


def capacity_rst(h, w, restart_rows=1):
    """`capacity` for a file with restart intervals (w2l_jpeg_capacity_rst): 6 more header bytes, and per interval a padding
    byte, its possible stuffed 00 and the marker"""
    n = int(_lib.load().w2l_jpeg_capacity_rst(int(h), int(w), int(restart_rows)))
    if n == 0:
        raise ValueError("jpeg: size %r x %r or restart_rows %r is out of range" % (h, w, restart_rows))
    return n


def header_rst(h, w, quality, restart_rows=1):
    """the 629 bytes in front of the entropy stream of a file with restart intervals (`header` plus the DRI segment)"""
    buf = (C.c_uint8 * HEADER_BYTES_RST)()
    _lib.check(_lib.load().w2l_jpeg_header_rst(int(h), int(w), int(quality), int(restart_rows), buf), "jpeg_header_rst")
    return bytes(buf)


ENCODE_SLOT_BYTES = 1 << 30       # encode_frames: device bytes of one launch's output slots (each holds the worst case)


def encode_frames(frames, quality=95, restart_rows=1, boxes=None, frame_index=None):
    """The frames of a Motion-JPEG stream: whole device frames (uint8 [N,H,W,3] BGR, or a list of such tensors / single frames),
    or with `boxes` their crops as in `encode_crops`, each as a complete JFIF file with a restart interval of `restart_rows` MCU
    rows - byte-equal to PIL's `save(format="JPEG", quality=quality, subsampling=2, restart_marker_rows=restart_rows)`.  Staging as
    `encode_crops`: one pinned copy in, two kernels, the lengths back, then the used bytes; frames whose worst-case slots would
    exceed ENCODE_SLOT_BYTES together are encoded in several such launches."""
    if restart_rows is None:
        raise ValueError("jpeg: encode_frames writes restart intervals (restart_rows >= 1); encode_crops writes files without")
    plan = _Plan(frames, boxes, quality, frame_index, restart_rows)
    per = max(1, ENCODE_SLOT_BYTES // plan.stride)
    if plan.n <= per:
        return plan.run()
    fl = _frame_list(frames)
    tensors = [_as_frame(f) for f in fl]
    bx = [(0, 0, f[3], f[2]) for f in fl] if boxes is None else list(boxes)
    idx = list(range(len(bx))) if frame_index is None else [int(i) for i in frame_index]
    out = []
    for i in range(0, len(bx), per):
        used = sorted(set(idx[i:i + per]))
        out += _Plan([tensors[j] for j in used], bx[i:i + per], quality, [used.index(j) for j in idx[i:i + per]], restart_rows).run()
    return out


def _as_frame(f):
    """the [H,W,3] view of one entry of `_frame_list`"""
    t, addr, H, W = f
    off = (addr - t.data_ptr()) // (H * W * 3)
    return t[off] if t.dim() == 4 else t


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


# ---------------------------------------------------------------- decoding
MALFORMED = -100                  # w2l_jpeg_parse: not a JPEG, or cut inside its header; the other reasons: outside the class
STATUS_TEXT = {-1: "bits that are no code of the file's Huffman table", -2: "a zero run past coefficient 63",
               -3: "a marker or left-over bytes before the end of the last MCU", -4: "the stream ends early",
               -5: "a row the launch cannot take"}


class UnsupportedJpeg(ValueError):
    """a well-formed JPEG file outside the class the device decodes (progressive, 4:4:4, grayscale, restart intervals, ...);
    `.code` is the parser's reason (W2L_JPEG_* of include/w2l_hip.h)"""

    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


def parse(data):
    """the _lib.JpegInfo of one file's bytes; UnsupportedJpeg for a file outside the class, plain ValueError for one that is no
    JPEG or is cut inside its header"""
    lib = _lib.load()
    info = _lib.JpegInfo()
    data = bytes(data)
    rc = lib.w2l_jpeg_parse(data, len(data), C.byref(info))
    if rc != 0:
        msg = (lib.w2l_last_error() or b"?").decode()
        if rc == MALFORMED or rc > MALFORMED:
            raise ValueError(msg)
        raise UnsupportedJpeg(msg, rc)
    return info


def probe(data):
    """(H, W) of a file the device decodes; raises UnsupportedJpeg with the parser's reason otherwise"""
    info = parse(data)
    return info.H, info.W


def _decode(datas, infos, device, segments=None):
    """(tensors, status int32 numpy [n]) of parsed files: one pinned buffer and one copy in, the kernels on the current stream,
    one copy of status back.  tensors[i] is complete where status[i] == 0.  segments: None for w2l_jpeg_decode_rows (one lane per
    file), or the JPEG_SEGMENT records of all files for w2l_jpeg_decode_rows_rst (one lane per record), staged in the same buffer."""
    import torch
    lib = _lib.load()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("jpeg: decode_files needs a HIP device (there is no host fallback), got %s" % device)
    n = len(datas)
    if n < 1 or n > MAX_ROWS:
        raise ValueError("jpeg: %d files in one batch (1 .. %d)" % (n, MAX_ROWS))
    tb = int(lib.w2l_jpeg_table_bytes())
    sets, table = {}, np.zeros(n, JPEG_ROW)
    for i, info in enumerate(infos):
        key = C.string_at(C.addressof(info) + 20, C.sizeof(_lib.JpegInfo) - 20)    # nvals, quant, bits, vals
        if key not in sets:
            buf = (C.c_uint8 * tb)()
            rc = lib.w2l_jpeg_build_tables(C.byref(info), buf)
            if rc != 0:
                raise ValueError("jpeg: file %d: %s" % (i, (lib.w2l_last_error() or b"?").decode()))
            sets[key] = (len(sets), bytes(buf))
        table[i] = (0, 0, info.ecs_bytes, info.H, info.W, sets[key][0])
    max_blocks = int(max(blocks(h, w) for h, w in zip(table["H"], table["W"])))
    if max_blocks > MAX_BLOCKS:
        raise ValueError("jpeg: a file of %d blocks (at most %d)" % (max_blocks, MAX_BLOCKS))
    src_off = np.concatenate([[0], np.cumsum(table["nbytes"].astype(np.int64))])
    dst_off = np.concatenate([[0], np.cumsum(table["H"].astype(np.int64) * table["W"] * 3)])
    with torch.cuda.device(device):
        # ---- one staging buffer: [rows][table sets][segments][the files' entropy-coded segments, back to back]
        st = Staging(device)
        rows, tabs = st.table(JPEG_ROW, n), st.reserve(tb * len(sets))
        segs = st.table(JPEG_SEGMENT, 0 if segments is None else len(segments))
        ecs = st.reserve(int(src_off[-1]), boundary=1)
        st.allocate()
        out = torch.empty(int(dst_off[-1]), dtype=torch.uint8, device=device)
        table["src"] = st.address(ecs) + src_off[:-1]
        table["dst"] = out.data_ptr() + dst_off[:-1]
        st.view(rows)[:] = table
        tabs_host, ecs_host = st.view(tabs), st.view(ecs)
        for idx, blob in sets.values():
            tabs_host[idx * tb:(idx + 1) * tb] = np.frombuffer(blob, np.uint8)
        for i, (d, info) in enumerate(zip(datas, infos)):
            ecs_host[src_off[i]:src_off[i + 1]] = np.frombuffer(d, np.uint8, info.ecs_bytes, info.ecs_offset)
        if segments is not None:
            st.view(segs)[:] = segments
        st.upload()                                                             # one copy in
        status = torch.empty(n, dtype=torch.int32, device=device)
        if segments is None:
            ws_bytes = int(lib.w2l_jpeg_decode_workspace_bytes(n, max_blocks))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            _lib.check(lib.w2l_jpeg_decode_rows(_lib.current_stream(), n, _lib.ptr(st.dev), C.c_void_p(st.address(tabs)), len(sets),
                                                max_blocks, _lib.ptr(status), _lib.ptr(ws), ws_bytes), "jpeg_decode_rows")
        else:
            ws_bytes = int(lib.w2l_jpeg_decode_workspace_bytes_rst(n, max_blocks))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            _lib.check(lib.w2l_jpeg_decode_rows_rst(_lib.current_stream(), n, _lib.ptr(st.dev), C.c_void_p(st.address(tabs)),
                                                    len(sets), max_blocks, C.c_void_p(st.address(segs)), len(segments),
                                                    _lib.ptr(status), _lib.ptr(ws), ws_bytes), "jpeg_decode_rows_rst")
        st = status.cpu().numpy()                                               # one copy back (waits for the kernels)
    imgs = [out[int(dst_off[i]):int(dst_off[i + 1])].view(int(table["H"][i]), int(table["W"][i]), 3) for i in range(n)]
    return imgs, st


def decode_files(datas, device):
    """The images of JPEG files given as bytes: a list of device uint8 [H,W,3] BGR tensors (cv2.imread's order), views of one
    buffer, byte-equal to `np.asarray(Image.open(BytesIO(d)).convert("RGB"))[:, :, ::-1]`.  Runs on the current stream of `device`.
    UnsupportedJpeg (from `probe`'s parser) for a file outside the class the device decodes, ValueError naming the index and the
    reason for a file whose stream the kernel refuses; RuntimeError for a CPU device."""
    import torch
    if torch.device(device).type != "cuda":
        raise RuntimeError("jpeg: decode_files needs a HIP device (there is no host fallback), got %s" % (device,))
    datas = [bytes(d) for d in datas]
    infos = []
    for i, d in enumerate(datas):
        try:
            infos.append(parse(d))
        except UnsupportedJpeg as e:
            raise UnsupportedJpeg("jpeg: file %d: %s" % (i, e), e.code) from None
        except ValueError as e:
            raise ValueError("jpeg: file %d: %s" % (i, e)) from None
    imgs, st = _decode(datas, infos, device)
    if (st != 0).any():
        i = int(np.flatnonzero(st)[0])
        raise ValueError("jpeg: file %d is corrupt: %s (status %d)" % (i, STATUS_TEXT.get(int(st[i]), "?"), int(st[i])))
    return imgs


# ---------------------------------------------------------------- Motion-JPEG frames: files with restart intervals
class CorruptJpeg(ValueError):
    """a frame of `decode_frames` that is cut, whose restart markers are wrong or whose stream the kernel refuses; `.index` is its
    position in the call's list"""

    def __init__(self, msg, index):
        super().__init__(msg)
        self.index = index


def parse_frame(data):
    """(the _lib.JpegInfo, Ri) of one frame's bytes: `parse` for the same class plus a restart interval of Ri MCUs (0: none), the
    class `decode_frames` takes.  Raises as `parse` does."""
    lib = _lib.load()
    info, ri = _lib.JpegInfo(), C.c_int32(0)
    data = bytes(data)
    rc = lib.w2l_jpeg_parse_rst(data, len(data), C.byref(info), C.byref(ri))
    if rc != 0:
        msg = (lib.w2l_last_error() or b"?").decode()
        if rc == MALFORMED or rc > MALFORMED:
            raise ValueError(msg)
        raise UnsupportedJpeg(msg, rc)
    return info, int(ri.value)


def restart_segments(data, info, ri):
    """the JPEG_SEGMENT records (row = 0) of a parsed frame: one per restart interval, found by the host's linear marker scan
    (w2l_jpeg_restart_segments); ValueError where the markers' count or order is wrong"""
    lib = _lib.load()
    n_mcus = (-(-info.H // 16)) * (-(-info.W // 16))
    n = -(-n_mcus // ri) if ri > 0 else 1
    out = np.zeros(n, JPEG_SEGMENT)
    ecs = np.frombuffer(data, np.uint8, info.ecs_bytes, info.ecs_offset)
    rc = lib.w2l_jpeg_restart_segments(C.c_void_p(ecs.ctypes.data), info.ecs_bytes, int(ri), n_mcus, C.c_void_p(out.ctypes.data), n)
    if rc != n:
        raise ValueError((lib.w2l_last_error() or b"?").decode() if rc < 0 else "jpeg: %d restart intervals, expected %d" % (rc, n))
    return out


def decode_frames(datas, device):
    """`decode_files` for the frames of a Motion-JPEG stream: files with restart intervals and files without share one launch
    (w2l_jpeg_decode_rows_rst: one lane per interval; a file without is one interval).  A list of device uint8 [H,W,3] BGR
    tensors, views of one buffer, byte-equal to PIL's decode.  UnsupportedJpeg for a frame outside the class, ValueError naming
    the frame index for one that is cut, whose markers are wrong or whose stream the kernel refuses; RuntimeError for a CPU device."""
    import torch
    if torch.device(device).type != "cuda":
        raise RuntimeError("jpeg: decode_frames needs a HIP device (there is no host fallback), got %s" % (device,))
    datas = [bytes(d) for d in datas]
    infos, segs = [], []
    for i, d in enumerate(datas):
        try:
            info, ri = parse_frame(d)
            s = restart_segments(d, info, ri)
        except UnsupportedJpeg as e:
            raise UnsupportedJpeg("jpeg: frame %d: %s" % (i, e), e.code) from None
        except ValueError as e:
            raise CorruptJpeg("jpeg: frame %d is corrupt: %s" % (i, e), i) from None
        s["row"] = i
        infos.append(info)
        segs.append(s)
    imgs, st = _decode(datas, infos, device, np.concatenate(segs))
    if (st != 0).any():
        i = int(np.flatnonzero(st)[0])
        raise CorruptJpeg("jpeg: frame %d is corrupt: %s (status %d)" % (i, STATUS_TEXT.get(int(st[i]), "?"), int(st[i])), i)
    return imgs
