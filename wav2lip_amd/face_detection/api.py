"""`FaceAlignment` (face_detection/api.py:41-77) over the HIP S3FD detector: `get_detections_for_batch(images)` takes the
reference's numpy uint8 BGR batch [B,H,W,3] and returns one (x1, y1, x2, y2) int tuple or None per image.  `precision="bf16"`
(opt-in) runs the detector network on its bf16-storage graph; the gate, NMS and thresholds are the same.  `det_scale=k` (opt-in,
1..8) runs it on the frames at (H // k, W // k) and maps every rect back to the full frame: x * float32(W / (W // k)),
y * float32(H / (H // k)), then the clip at 0 and int() of api.py:61-77 as before."""
import os
from enum import Enum

import numpy as np
import torch

from .s3fd import (RECT_FOUND, RECT_HOST, check_det_scale, det_rect_scale, det_size, first_rects, nms, nms_batch, s3fd,
                   scale_box)


class LandmarksType(Enum):
    _2D = 1
    _2halfD = 2
    _3D = 3


class NetworkSize(Enum):
    LARGE = 4

    def __int__(self):
        return self.value


DEFAULT_WEIGHTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s3fd.pth")   # detection/sfd/sfd_detector.py:17


class FaceAlignment:
    def __init__(self, landmarks_type=LandmarksType._2D, network_size=NetworkSize.LARGE, device="cuda", flip_input=False,
                 face_detector="sfd", verbose=False, path_to_detector=None, state_dict=None, precision="f32", det_scale=1):
        from ..models.wav2lip import check_precision
        self.precision = check_precision(precision)
        self.det_scale = check_det_scale(det_scale)
        if face_detector != "sfd":
            raise NotImplementedError("only the 'sfd' detector of the reference is mirrored")
        if not torch.cuda.is_available() or "cuda" not in str(device):
            raise RuntimeError("wav2lip_amd.face_detection: needs a HIP device (no CPU path)")
        self.device, self.flip_input, self.landmarks_type, self.verbose = device, flip_input, landmarks_type, verbose
        net = s3fd()
        if state_dict is None:
            path = path_to_detector or DEFAULT_WEIGHTS
            if not os.path.isfile(path):
                raise FileNotFoundError("S3FD weights %s not found (the reference downloads s3fd-619a316812.pth, "
                                        "sfd_detector.py:10-24; there is no network here): pass path_to_detector or "
                                        "state_dict" % path)
            state_dict = torch.load(path, map_location="cpu")
        net.load_state_dict(state_dict)
        self.face_detector = net.to(device).eval()

    def _scale_kw(self):
        """the keyword `dense_boxes` / `dense_boxes_rows` take for a reduced detection frame: none at scale 1"""
        k = getattr(self, "det_scale", 1)
        return {} if k == 1 else {"det_scale": k}

    def rect_scale(self, H, W):
        """(sx, sy) that map a rect of the detection frame back to an H x W frame (`s3fd.det_rect_scale`); None at scale 1.
        ValueError when the reduced frame would be too small for the network."""
        k = getattr(self, "det_scale", 1)
        return None if k == 1 else det_rect_scale(H, W, *det_size(H, W, k))

    def _batch_scale(self, images):
        """`rect_scale` for a batch [B,H,W,3]; at scale 1 it is None and the batch is not looked at"""
        return None if getattr(self, "det_scale", 1) == 1 else self.rect_scale(*images.shape[1:3])

    def detect_from_batch(self, images_bgr):
        """sfd_detector.py:39-45 semantics per image: candidates (score > 0.05), NMS 0.3, keep score > 0.5.
        images: numpy uint8 [B,H,W,3] BGR (or a torch uint8 tensor already on the device).  At det_scale > 1 the boxes come back in
        full-frame coordinates (`s3fd.scale_box`); the scores are the detector's."""
        scale = self._batch_scale(images_bgr)
        if isinstance(images_bgr, np.ndarray):
            images_bgr = torch.from_numpy(np.ascontiguousarray(images_bgr)).to(self.device)
        with torch.no_grad():
            levels = self.face_detector.dense_boxes(images_bgr, precision=self.precision, **self._scale_kw())
            table = torch.cat(levels, dim=1).contiguous()       # [B, sum FH*FW, 5]
            keep, counts = nms_batch(table, 0.05, 0.3)          # gate + NMS on the device: only the survivors cross PCIe
            counts_h = counts.cpu().tolist()
            out = []
            for b, n in enumerate(counts_h):
                d = table[b].index_select(0, keep[b, :n].long()).cpu().numpy()
                if scale is not None:
                    d[:, :4] = scale_box(d[:, :4], *scale)
                out.append([x for x in d if x[-1] > 0.5])
        return out

    def _candidates(self, images_bgr, rows=None, resolve=True):
        """the batch's box table [B, P, 5] and its gated NMS (keep, counts), all on the device: the one place the detector's boxes
        come from, for `get_detections_for_batch`, `get_candidates_for_batch`, `rects_for_rows` and `cands_for_rows` (a test that
        prescribes a box table overrides this).  `rows` = (B, H, W): `images_bgr` is a device address table of B frames
        (`s3fd.dense_boxes_rows`) and nothing is read back - an image whose NMS overflowed keeps counts = -1, which the rect
        kernels flag RECT_HOST; `resolve=False` asks the same of a batch of images."""
        if rows is not None:
            B, H, W = rows
            levels = self.face_detector.dense_boxes_rows(images_bgr, B, H, W, precision=self.precision, **self._scale_kw())
            table = torch.cat(levels, dim=1).contiguous()
            keep, counts = nms_batch(table, 0.05, 0.3, host_overflow=False)
            return table, keep, counts
        if isinstance(images_bgr, np.ndarray):
            images_bgr = torch.from_numpy(np.ascontiguousarray(images_bgr)).to(self.device)
        levels = self.face_detector.dense_boxes(images_bgr, precision=self.precision, **self._scale_kw())
        table = torch.cat(levels, dim=1).contiguous()           # [B, sum FH*FW, 5]
        keep, counts = nms_batch(table, 0.05, 0.3, host_overflow=resolve)
        return table, keep, counts

    def rects_for_rows(self, frames, B, H, W, rects, flags, offset):
        """`get_detections_for_batch` for the B frames of a device address table (`s3fd.dense_boxes_rows`), left on the device:
        rows [offset, offset + B) of the int32 arenas `rects` [R,4] = (x1, y1, x2, y2) and `flags` [R] receive what
        `w2l_s3fd_first_rect` writes.  No host read: an image whose NMS overflowed is flagged RECT_HOST like any other the device
        does not decide (face_detection/many.py re-runs that clip through `inference.face_detect`).  At det_scale > 1 the rects are
        full-frame coordinates (`w2l_s3fd_first_rect_scaled`)."""
        from .._lib import check, current_stream, load
        scale = self.rect_scale(H, W)
        if (rects.dtype != torch.int32 or flags.dtype != torch.int32 or not rects.is_contiguous() or not flags.is_contiguous()
                or rects.dim() != 2 or rects.shape[1] != 4 or flags.dim() != 1 or flags.shape[0] != rects.shape[0]
                or offset < 0 or offset + B > rects.shape[0]):
            raise ValueError("rects_for_rows: int32 arenas [R,4] and [R] with rows [%d, %d) inside them" % (offset, offset + B))
        with torch.no_grad():
            table, keep, counts = self._candidates(frames, rows=(B, H, W))
            out = (rects.data_ptr() + 16 * offset, flags.data_ptr() + 4 * offset)
            if scale is None:
                check(load().w2l_s3fd_first_rect(current_stream(), B, table.shape[1], table.data_ptr(), keep.data_ptr(),
                                                 counts.data_ptr(), 0.5, *out), "s3fd_first_rect")
            else:
                check(load().w2l_s3fd_first_rect_scaled(current_stream(), B, table.shape[1], table.data_ptr(), keep.data_ptr(),
                                                        counts.data_ptr(), 0.5, float(scale[0]), float(scale[1]), *out),
                      "s3fd_first_rect_scaled")

    def _top_rects(self, who, B, scale, cands, ncand, flags, offset, K, candidates):
        """the arena check and the one `w2l_s3fd_top_rects` call of `cands_for_rows` / `cands_for_batch` (`who` names the caller in
        the error); `scale`: the batch's `rect_scale`; `candidates()`: its `_candidates`"""
        from .._lib import check, current_stream, load
        scale = scale or (1.0, 1.0)
        if (any(t.dtype != torch.int32 or not t.is_contiguous() for t in (cands, ncand, flags)) or cands.dim() != 3
                or tuple(cands.shape[1:]) != (K, 4) or ncand.dim() != 1 or flags.dim() != 1
                or not ncand.shape[0] == flags.shape[0] == cands.shape[0] or offset < 0 or offset + B > cands.shape[0]):
            raise ValueError("%s: int32 arenas [R,%d,4], [R] and [R] with rows [%d, %d) inside them" % (who, K, offset, offset + B))
        with torch.no_grad():
            table, keep, counts = candidates()
            check(load().w2l_s3fd_top_rects(current_stream(), B, table.shape[1], table.data_ptr(), keep.data_ptr(), counts.data_ptr(),
                                            0.5, float(scale[0]), float(scale[1]), K, cands.data_ptr() + 16 * K * offset,
                                            ncand.data_ptr() + 4 * offset, flags.data_ptr() + 4 * offset), "s3fd_top_rects")

    def cands_for_rows(self, frames, B, H, W, cands, ncand, flags, offset, K):
        """the device-resident twin of `rects_for_rows` for tracked face selection (`face_detection/track.py`): rows [offset,
        offset + B) of the int32 arenas `cands` [R,K,4], `ncand` [R] and `flags` [R] receive what `w2l_s3fd_top_rects` writes - up to
        K candidate rects per frame, in full-frame coordinates at det_scale > 1.  No host read."""
        self._top_rects("cands_for_rows", B, self.rect_scale(H, W), cands, ncand, flags, offset, K,
                        lambda: self._candidates(frames, rows=(B, H, W)))

    def cands_for_batch(self, images, cands, ncand, flags, offset, K):
        """`cands_for_rows` for a batch of images given as `get_detections_for_batch` takes them (numpy uint8 BGR [B,H,W,3]): the
        arenas' rows [offset, offset + B) are written, the candidates stay on the device and nothing is read back (an image whose
        NMS overflowed is flagged RECT_HOST)"""
        self._top_rects("cands_for_batch", len(images), self._batch_scale(images), cands, ncand, flags, offset, K,
                        lambda: self._candidates(images, resolve=False))

    def get_candidates_for_batch(self, images, K):
        """up to K candidate rects per image - `get_detections_for_batch`'s rect is the first of them: a list of (x1, y1, x2, y2)
        int tuples per image, from one launch (`w2l_s3fd_top_rects`) and one copy back per batch; an image the device flags takes
        `track.host_top_rects`, which raises what Python's int() raises."""
        from .s3fd import top_rects
        from .track import host_top_rects
        scale = self._batch_scale(images)
        with torch.no_grad():
            table, keep, counts = self._candidates(images)
            cands, ncand, flags = top_rects(table, keep, counts, 0.5, K, scale)
            out = []
            for b in range(len(flags)):
                if flags[b] == RECT_HOST:
                    out.append(host_top_rects(table[b].cpu().numpy(), keep[b].cpu().numpy(), int(counts[b].item()), K, scale))
                else:
                    out.append([tuple(int(v) for v in c) for c in cands[b, :ncand[b]]])
        return out

    def get_detections_for_batch(self, images):
        """api.py:61-77 (the BGR->RGB flip of :62 happens inside the device pack kernel).  The rect of every image comes from one
        launch (`w2l_s3fd_first_rect`) and one copy back per batch; an image the device flags (a non-finite or huge coordinate)
        takes the per-image host rule below, which raises what Python's int() raises there.  At det_scale > 1 both map the row back
        to the full frame first, by the same float32 multiply."""
        scale = self._batch_scale(images)

        def first_rect(dets):
            # the best-scoring detection, clipped at the image origin and truncated to ints; None when nothing survived NMS
            if len(dets) == 0:
                return None
            box = dets[0][:4] if scale is None else scale_box(dets[0][:4], *scale)
            box = np.maximum(np.asarray(box), 0)
            return tuple(int(v) for v in box)

        with torch.no_grad():
            table, keep, counts = self._candidates(images)
            res = first_rects(table, keep, counts, 0.5, scale)
            out = []
            for b, r in enumerate(res):
                if r[4] == RECT_HOST:
                    n = int(counts[b].item())
                    d = table[b].index_select(0, keep[b, :n].long()).cpu().numpy()
                    out.append(first_rect([x for x in d if x[-1] > 0.5]))
                else:
                    out.append(tuple(int(v) for v in r[:4]) if r[4] == RECT_FOUND else None)
        return out
