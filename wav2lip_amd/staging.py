"""The staging buffer of the packed paths, laid out once.

Every packed path (multiclip, evaluation, face_detection/many, streaming, jpeg, real_videos_inference) feeds its kernels the same
way: a few tables of C structs (the dtypes of `_lib`) and some raw blobs are laid out in ONE host buffer, the buffer goes up in
ONE copy, and the kernels get device addresses into it.  A reservation starts on a 16-byte boundary unless it asks for another
(the tables must, include/w2l_hip.h; jpeg packs its entropy segments back to back), and the buffer's size is rounded up to 16.

    st = Staging(device)                     # pinned host memory when the device is a GPU
    rows = st.table(FRAME_ROW, n)            # reserve; the calls' order is the buffer's order
    src = st.place(frames)                   # a host array (or a list of arrays of one shape): a blob that `allocate` fills;
                                             # something on the device already: nothing reserved, it is read where it lies
    raw = st.reserve(nbytes, boundary=1)
    st.allocate()                            # the one host and the one device buffer
    st.view(rows)[r] = (st.address(src), ...)    # `view`: the handle's part of the host buffer as a numpy array of its dtype
    st.upload()                              # the one copy, non-blocking from pinned memory

`address(h)` / `host_address(h)` are the addresses a kernel / a host-side check gets, `tensor(h)` is the handle's bytes as a
device tensor; `st.host` and `st.dev` are the two buffers (`PipelinedRunner`'s `upload=` takes them) and `st.residents` the device
objects that were placed, which a launch must keep alive.  Nothing is allocated before `allocate`, so a layout can be computed
for its own sake (`multiclip.staging_layout`).
"""
import numpy as np
import torch

ALIGN = 16           # tables start on a 16-byte boundary (include/w2l_hip.h), and so does everything else by default
ADDRESS = np.dtype("<u8")    # the entry of a table of bare device addresses (the detector's row tables)


def align(n, boundary=ALIGN):
    return (n + boundary - 1) // boundary * boundary


class Region:
    """a handle: `nbytes` bytes at `offset` of the staging buffer, seen as `dtype`; or, with `resident` set, `nbytes` bytes at
    byte `offset` of that device object (anything with `data_ptr()` and `nbytes`), which are not part of the buffer"""
    __slots__ = ("offset", "nbytes", "dtype", "resident")

    def __init__(self, offset, nbytes, dtype=np.uint8, resident=None):
        self.offset, self.nbytes, self.dtype, self.resident = offset, nbytes, dtype, resident


class Staging:
    def __init__(self, device):
        self.device = torch.device(device)
        self.pinned = self.device.type == "cuda"
        self.nbytes = 0              # the end of the last reservation
        self.host = self.dev = None
        self._residents = {}         # id -> device object `place` was given
        self.placed = []             # (handle, host data) that `allocate` copies in

    # ---- the layout: nothing is allocated
    def reserve(self, nbytes, boundary=ALIGN, dtype=np.uint8):
        h = Region(align(self.nbytes, boundary), nbytes, dtype)
        self.nbytes = h.offset + h.nbytes
        return h

    def table(self, dtype, n):
        return self.reserve(n * dtype.itemsize, dtype=dtype)

    def place(self, x, index=None):
        """`x`, or with `index` its element `x[index]`: host data (an array, or a list of arrays of one shape, which become one
        contiguous blob) is reserved and copied in by `allocate`; what is on the device already is read where it lies"""
        if hasattr(x, "data_ptr"):
            self._residents[id(x)] = x
            if index is None:
                return Region(0, x.nbytes, resident=x)
            each = x.nbytes // x.shape[0]
            return Region(index * each, each, resident=x)
        if index is not None:
            x = np.asarray(x[index])
        h = Region(align(self.nbytes), sum(f.nbytes for f in x) if type(x) is list else x.nbytes)     # `reserve`, spelled out
        self.nbytes = h.offset + h.nbytes
        self.placed.append((h, x))
        return h

    @property
    def size(self):
        """bytes of the buffer: the reservations so far, rounded up"""
        return align(self.nbytes)

    @property
    def residents(self):
        return tuple(self._residents.values())

    # ---- the buffers
    def allocate(self):
        self.host = torch.empty(self.size, dtype=torch.uint8, pin_memory=self.pinned)
        self.dev = torch.empty(self.size, dtype=torch.uint8, device=self.device)
        host = self._bytes = self.host.numpy()
        self._base = self.dev.data_ptr()
        for h, x in self.placed:                         # once per staged blob of a tick: kept lean
            if type(x) is list:
                dst = host[h.offset:h.offset + h.nbytes]
                for i, f in enumerate(x):
                    dst[i * f.nbytes:(i + 1) * f.nbytes].view(f.dtype).reshape(f.shape)[...] = f
            else:
                host[h.offset:h.offset + h.nbytes] = x.reshape(-1).view(np.uint8)
        self.placed = []

    def view(self, h):
        return self._bytes[h.offset:h.offset + h.nbytes].view(h.dtype)

    def address(self, h):
        return (self._base if h.resident is None else h.resident.data_ptr()) + h.offset

    def host_address(self, h):
        return self.host.data_ptr() + h.offset

    def tensor(self, h):
        """the handle's bytes as a uint8 device tensor: a slice of the device buffer, or of the tensor that was placed"""
        flat = self.dev if h.resident is None else h.resident.view(-1).view(torch.uint8)
        return flat[h.offset:h.offset + h.nbytes]

    def upload(self):
        self.dev.copy_(self.host, non_blocking=self.pinned)
