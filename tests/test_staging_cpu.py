"""The staging-buffer builder (wav2lip_amd/staging.py) on torch.device("cpu"), unpinned: where reservations land, what `place`
does with host data and with what lies on the device already, that a view written through a handle is the host buffer at the
handle's offset, and that `upload` is one copy."""
import numpy as np
import torch

from wav2lip_amd import _lib, staging
from wav2lip_amd.staging import Staging

CPU = torch.device("cpu")


def test_align_rounds_up_to_the_boundary():
    assert [staging.align(n) for n in (0, 1, 15, 16, 17, 32)] == [0, 16, 16, 16, 32, 32]
    assert [staging.align(n, 1) for n in (0, 1, 17)] == [0, 1, 17] and staging.align(9, 8) == 16


def test_offsets_of_mixed_tables_and_blobs():
    """every reservation starts on the next 16-byte boundary behind the one before it: what the hand-written
    `off = _align(off + nbytes)` chains gave"""
    st = Staging(CPU)
    assert not st.pinned and st.size == 0
    rows = st.table(_lib.FRAME_ROW, 3)                     # 144 bytes
    mels = st.table(_lib.MEL_ROW, 3)                       # 48
    blobs = [st.reserve(n) for n in (0, 1, 15, 16, 17)]
    segs = st.table(_lib.LSE_SEGMENT, 3)                   # 24: no multiple of 16
    last = st.reserve(5)
    assert (rows.offset, rows.nbytes, mels.offset, mels.nbytes) == (0, 144, 144, 48)
    want, off = [], 192
    for n in (0, 1, 15, 16, 17):
        want.append(off)
        off = (off + n + 15) // 16 * 16
    assert [b.offset for b in blobs] == want == [192, 192, 208, 224, 240]
    assert [b.nbytes for b in blobs] == [0, 1, 15, 16, 17]
    assert (segs.offset, last.offset) == (272, 304) and st.nbytes == 309 and st.size == 320
    assert all(h.offset % 16 == 0 for h in [rows, mels, segs, last] + blobs)
    st.allocate()
    assert st.host.numel() == st.dev.numel() == 320 and not st.host.is_pinned() and st.dev.device == CPU
    assert st.view(rows).dtype == _lib.FRAME_ROW and st.view(rows).shape == (3,) and st.view(blobs[0]).shape == (0,)


def test_an_empty_table_takes_no_room_and_keeps_the_boundary():
    st = Staging(CPU)
    st.reserve(3)
    empty = st.table(_lib.JPEG_SEGMENT, 0)
    after = st.reserve(4)
    assert (empty.offset, empty.nbytes, after.offset) == (16, 0, 16)
    st.allocate()
    assert st.view(empty).shape == (0,) and st.view(empty).dtype == _lib.JPEG_SEGMENT and st.tensor(empty).numel() == 0
    assert st.address(empty) == st.dev.data_ptr() + 16


def test_unaligned_blobs_lie_back_to_back():
    st = Staging(CPU)
    rows = st.table(_lib.JPEG_ROW, 1)
    packed = [st.reserve(n, boundary=1) for n in (5, 0, 7, 1)]
    aligned = st.reserve(2)
    assert [p.offset for p in packed] == [32, 37, 37, 44] and aligned.offset == 48 and rows.offset == 0
    assert st.size == 64


def test_place_copies_host_data_in_and_reads_device_data_where_it_lies():
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (3, 5, 3), dtype=np.uint8) for _ in range(4)]        # 45 bytes each
    samples = rng.standard_normal(7).astype(np.float32)
    clip = rng.integers(0, 256, (4, 3, 5, 3), dtype=np.uint8)
    resident = torch.arange(2 * 3 * 5 * 3, dtype=torch.uint8).reshape(2, 3, 5, 3)

    class Window:                                           # anything with data_ptr() and nbytes (streaming.Resident)
        nbytes = 12

        @staticmethod
        def data_ptr():
            return resident.data_ptr() + 8

    st = Staging(CPU)
    table = st.table(_lib.MEL_ROW, 2)
    a, b, c = st.place(frames), st.place(samples), st.place(clip, 2)
    before = st.nbytes
    d, e, f = st.place(resident), st.place(resident, 1), st.place(Window)
    assert st.nbytes == before                              # nothing reserved for what is on the device already
    assert (a.offset, a.nbytes, b.offset, b.nbytes, c.offset, c.nbytes) == (32, 180, 224, 28, 256, 45)
    assert [f is resident for f in st.residents] == [True, False] and st.residents[1] is Window
    st.allocate()
    host = st.host.numpy()
    assert np.array_equal(host[32:212].reshape(4, 3, 5, 3), np.stack(frames))          # a list: one contiguous blob
    assert np.array_equal(host[224:252].view(np.float32), samples)
    assert np.array_equal(host[256:301].reshape(3, 5, 3), clip[2])
    assert st.address(a) == st.dev.data_ptr() + 32 and st.host_address(a) == st.host.data_ptr() + 32
    assert st.address(d) == resident.data_ptr() and (d.nbytes, e.nbytes) == (90, 45)
    assert st.address(e) == resident.data_ptr() + 45 and st.address(f) == resident.data_ptr() + 8
    assert torch.equal(st.tensor(e).view(3, 5, 3), resident[1]) and st.tensor(e).data_ptr() == st.address(e)
    assert st.tensor(table).data_ptr() == st.dev.data_ptr() and st.tensor(table).numel() == 32


def test_a_view_written_through_a_handle_lands_at_its_offset_and_upload_copies_once():
    st = Staging(CPU)
    st.reserve(5)
    rows = st.table(_lib.MEL_ROW, 3)
    caps = st.reserve(8, dtype=np.int32)
    st.allocate()
    st.host.zero_()
    copies = []
    real = st.dev.copy_
    st.dev.copy_ = lambda src, non_blocking=False: copies.append(non_blocking) or real(src, non_blocking=non_blocking)
    st.view(rows)[1] = (0x1122334455667788, 7, -2)
    st.view(rows)["T"][2:] = 9
    st.view(caps)[:] = (3, 4)
    at = st.host.numpy()[rows.offset:]
    assert rows.offset == 16 and at[:16].tolist() == [0] * 16
    assert at[16:32].tolist() == [0x88, 0x77, 0x66, 0x55, 0x44, 0x33, 0x22, 0x11, 7, 0, 0, 0, 0xfe, 0xff, 0xff, 0xff]
    assert at[40:44].tolist() == [9, 0, 0, 0] and st.host.numpy()[caps.offset:caps.offset + 8].view(np.int32).tolist() == [3, 4]
    st.upload()
    assert copies == [False]                                # one copy; blocking, since nothing is pinned here
    assert torch.equal(st.dev, st.host) and st.dev.data_ptr() != st.host.data_ptr()
