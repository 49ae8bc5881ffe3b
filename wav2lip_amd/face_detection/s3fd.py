"""`s3fd` (face_detection/detection/sfd/net_s3fd.py:22-129) with the reference's attribute names and state-dict keys, run as
fused HIP launches: every convolution is a `w2l_conv` layer (bias + ReLU folded into the launch; 3x3 / stride 1 layers go
through the Winograd kernel), max-pools, L2Norm and the box decode are the glue kernels of csrc/detect.hip.
Activations are NHWC fp32; the detection heads write (conf, loc) maps that `w2l_s3fd_decode` turns into dense
(x1, y1, x2, y2, score) tables, one per pyramid level.

`dense_boxes(images, precision="bf16")` runs the graph in bf16 storage instead (opt-in): bf16 NHWC activations, the
convolutions as `w2l_convb` launches (bias as the fp32 shift, ReLU), the bf16 instantiations of the same glue kernels and one fused
head per level (`w2l_s3fd_headb_decode`, csrc/detect_bf16.hip: conf + loc contraction and decode, the logits never leave the chip).

`det_scale=k` (opt-in, 1..8) runs either graph on the frame at (H // k, W // k) - `cv2.resize(frame, (w // k, h // k))`, the sizes
of inference.py:202-203 - which `w2l_s3fd_pack_rows_scaled` computes while it fills the graph's input; the tables stay in the
reduced frame's coordinates and `det_rect_scale` gives the two fp32 factors that map a rect back."""
import ctypes as C

import numpy as np
import torch
from torch import nn

from .. import bf16, engine
from .._lib import ACT_NONE, ACT_RELU, check, current_stream, load, ptr

# (name, cin, cout, kernel, stride, padding), net_s3fd.py:25-48
BACKBONE = [("conv1_1", 3, 64, 3, 1, 1), ("conv1_2", 64, 64, 3, 1, 1), "pool",
            ("conv2_1", 64, 128, 3, 1, 1), ("conv2_2", 128, 128, 3, 1, 1), "pool",
            ("conv3_1", 128, 256, 3, 1, 1), ("conv3_2", 256, 256, 3, 1, 1), ("conv3_3", 256, 256, 3, 1, 1), "tap:conv3_3", "pool",
            ("conv4_1", 256, 512, 3, 1, 1), ("conv4_2", 512, 512, 3, 1, 1), ("conv4_3", 512, 512, 3, 1, 1), "tap:conv4_3", "pool",
            ("conv5_1", 512, 512, 3, 1, 1), ("conv5_2", 512, 512, 3, 1, 1), ("conv5_3", 512, 512, 3, 1, 1), "tap:conv5_3", "pool",
            ("fc6", 512, 1024, 3, 1, 3), ("fc7", 1024, 1024, 1, 1, 0), "tap:fc7",
            ("conv6_1", 1024, 256, 1, 1, 0), ("conv6_2", 256, 512, 3, 2, 1), "tap:conv6_2",
            ("conv7_1", 512, 128, 1, 1, 0), ("conv7_2", 128, 256, 3, 2, 1), "tap:conv7_2"]
# (feature, L2Norm module or None, conf channels), net_s3fd.py:50-66
HEADS = [("conv3_3", "conv3_3_norm", 4), ("conv4_3", "conv4_3_norm", 2), ("conv5_3", "conv5_3_norm", 2), ("fc7", None, 2),
         ("conv6_2", None, 2), ("conv7_2", None, 2)]


class L2Norm(nn.Module):
    """parameter container of net_s3fd.py:6-19 (`weight` initialised to `scale`)"""

    def __init__(self, n_channels, scale=1.0):
        super().__init__()
        self.n_channels, self.scale, self.eps = n_channels, scale, 1e-10
        self.weight = nn.Parameter(torch.full((n_channels,), float(scale)))


MIN_FRAME = 32           # the smallest height / width the graph takes: five 2x2 max-pools, each of at least 2 x 2 (_Graph)
MAX_DET_SCALE = 8


def check_det_scale(k):
    """`det_scale` as an int in 1..MAX_DET_SCALE, or ValueError (a bool or a float is not an integer here)"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_DET_SCALE:
        raise ValueError("det_scale must be an integer in 1..%d, got %r" % (MAX_DET_SCALE, k))
    return int(k)


def det_size(H, W, k):
    """(Hd, Wd) = (H // k, W // k), the frame the detector sees at det_scale k (inference.py:202-203's sizes); ValueError when a
    reduced side falls below MIN_FRAME.  k = 1 returns (H, W) unchecked: that path is the graph's own business, as it was."""
    k = check_det_scale(k)
    if k == 1:
        return int(H), int(W)
    Hd, Wd = int(H) // k, int(W) // k
    if Hd < MIN_FRAME or Wd < MIN_FRAME:
        raise ValueError("det_scale=%d turns a %d x %d frame into %d x %d, below the %d x %d the S3FD graph needs (five 2x2 "
                         "max-pools)" % (k, H, W, Hd, Wd, MIN_FRAME, MIN_FRAME))
    return Hd, Wd


def det_rect_scale(H, W, Hd, Wd):
    """(sx, sy) = (float32(W / Wd), float32(H / Hd)): divided in double, rounded once - the factors of `scale_box`"""
    return np.float32(float(W) / float(Wd)), np.float32(float(H) / float(Hd))


def scale_box(box, sx, sy):
    """(x1, y1, x2, y2) of the reduced frame -> the full frame: x * sx, y * sy, one float32 multiply each (numpy float32 arrays
    multiply in float32) - what `w2l_s3fd_first_rect_scaled` does with `__fmul_rn` before its clip and truncation"""
    return np.asarray(box, dtype=np.float32) * np.array([sx, sy, sx, sy], dtype=np.float32)


def _bf16_buffer_sizes(B, H, W):
    """bytes of every buffer the bf16 _Graph would allocate for (B, H, W), computed from the shapes alone"""
    sizes = [2 * B * H * W * 8]                                   # packed input, 8 channels
    h, w, taps = H, W, {}
    for item in BACKBONE:
        if item == "pool":
            if h < 2 or w < 2:
                raise RuntimeError("image too small for the S3FD pyramid")
            h, w = h // 2, w // 2
            sizes.append(2 * B * h * w * c)
        elif isinstance(item, str):
            taps[item[4:]] = (h, w, c)
        else:
            _, _, c, k, st, p = item
            h, w = (h + 2 * p - k) // st + 1, (w + 2 * p - k) // st + 1
            if h < 1 or w < 1:
                raise RuntimeError("image too small for the S3FD pyramid")
            sizes.append(2 * B * h * w * bf16.round8(c))
    for feat, norm, _ in HEADS:
        fh, fw, c = taps[feat]
        if norm is not None:
            sizes.append(2 * B * fh * fw * c)
        sizes.append(4 * B * fh * fw * 5)                         # the level's dense table (fp32)
    return sizes


class _HeadB:
    """one pyramid level's conf + loc convolutions and box decode as ONE launch (w2l_s3fd_headb_*): weights rounded to bf16 once"""

    def __init__(self, conf, loc, ncls):
        self._lib = load()
        self.cin, self.ncls = conf.in_channels, ncls
        t = [conf.weight, conf.bias, loc.weight, loc.bias]
        self._keep = [p.detach().float().contiguous() if p is not None else None for p in t]
        h = C.c_void_p()
        check(self._lib.w2l_s3fd_headb_create(self.cin, ncls, *[ptr(p) for p in self._keep], current_stream(), C.byref(h)),
              "s3fd_headb_create")
        self.handle = h

    def decode(self, x, stride, out):
        """x: bf16.ActB features [B, FH, FW, >= cin]; out: float32 [B, FH*FW, 5]"""
        check(self._lib.w2l_s3fd_headb_decode(self.handle, current_stream(), x.N, x.H, x.W, stride, x.ptr, x.cs, ptr(out)),
              "s3fd_headb_decode")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.w2l_s3fd_headb_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _Graph:
    """buffers + launch list for one (batch, height, width) in one storage (engine.storage).  "f32": fp32 NHWC buffers, FusedConv
    plans, two head convolutions per level and `decode`.  "bf16", the opt-in bf16-storage detector: bf16 NHWC buffers, the backbone
    as convb plans (bias as the fp32 shift, ReLU), bf16 max-pools and L2Norms, one fused head per level writing the dense tables
    directly."""

    def __init__(self, model, B, H, W, device, precision="f32"):
        st = self.st = engine.storage(precision)
        self.precision = st.name
        if st is engine.BF16:
            big = max(_bf16_buffer_sizes(B, H, W))
            if big >= bf16.BUF_LIMIT:
                # checked before anything is allocated: inference.halving halves the batch on this error, as for fp32
                raise RuntimeError("S3FD bf16: a %d x %d x %d batch needs a %d-byte buffer, over the kernels' 2 GiB limit: split the "
                                   "batch" % (B, H, W, big))
        self.lib = lib = load()
        self.B, self.H, self.W = B, H, W
        self.x_in = st.new_buf(B, H, W, 4, device, zero=True)        # RGB + zero pad: 4 channels in fp32, 8 in bf16
        self.x_cs = self.x_in.shape[3]
        self.ops = []          # ("convs", Plan) | ("pool", src, dst) | ("l2norm", src, weight, dst) | ("head", _HeadB, src, stride, out)
        self.plans = []
        plan = None

        def flush():
            nonlocal plan
            if plan is not None:
                plan.tuned = st.shape_tuned
                self.ops.append(("convs", plan))
                self.plans.append(plan)
                plan = None

        def conv(name, src, act):
            nonlocal plan
            layer = st.layer_of(getattr(model, name), act, model._layers)
            ho, wo = layer.out_hw(src.H, src.W)
            ct = (layer.cout + 3) // 4 * 4          # fp32 rounds an output to 4 channels (bf16 buffers round to 8 and are zeroed anyway)
            dst = st.act(st.new_buf(B, ho, wo, ct, device, zero=(ct != layer.cout)), 0, layer.cout)
            if plan is None:
                plan = engine.Plan()
            st.record(plan, name, layer, src, dst)
            return dst

        x = st.act(self.x_in, 0, 3)
        taps = {}
        for item in BACKBONE:
            if item == "pool":
                flush()
                if x.H < 2 or x.W < 2:
                    raise RuntimeError("image too small for the S3FD pyramid")
                dst = st.act(st.new_buf(B, x.H // 2, x.W // 2, x.C, device), 0, x.C)
                self.ops.append(("pool", x, dst))
                x = dst
            elif isinstance(item, str):
                taps[item[4:]] = x
            else:
                x = conv(item[0], x, ACT_RELU)
        flush()
        self.levels = []       # fp32 only: (conf Act, loc Act, ncls, stride), what `decode` and s3fd.forward read
        self.dense = []
        for i, (feat, norm, ncls) in enumerate(HEADS):
            src, prefix = taps[feat], feat
            if norm is not None:
                flush()
                nb = st.act(st.new_buf(B, src.H, src.W, src.C, device), 0, src.C)
                self.ops.append(("l2norm", src, getattr(model, norm).weight, nb))
                src, prefix = nb, norm
            out = torch.empty((B, src.H * src.W, 5), device=device, dtype=torch.float32)
            if st is engine.F32:
                conf = conv(prefix + "_mbox_conf", src, ACT_NONE)
                loc = conv(prefix + "_mbox_loc", src, ACT_NONE)
                self.levels.append((conf, loc, ncls, 2 ** (i + 2)))
            else:
                head = _HeadB(getattr(model, prefix + "_mbox_conf"), getattr(model, prefix + "_mbox_loc"), ncls)
                self.ops.append(("head", head, src, 2 ** (i + 2), out))
            self.dense.append(out)
        flush()
        self._maxpool, self._l2norm = st.bind(lib, "maxpool2x2"), st.bind(lib, "l2norm_scale")
        self._pack, self._pack_rows = st.bind(lib, "s3fd_pack"), st.bind(lib, "s3fd_pack_rows")
        self._pack_rows_scaled = st.bind(lib, "s3fd_pack_rows_scaled")

    def pack(self, img):
        """`x_in` from contiguous uint8 [B,H,W,3] BGR frames on the device"""
        self._pack(current_stream(), self.B * self.H * self.W, ptr(img), ptr(self.x_in), self.x_cs)

    def pack_rows(self, frames, H, W, det_scale):
        """`x_in` from a device table of B frame addresses (uint8 [H,W,3] BGR each); det_scale > 1: resized to the graph's size"""
        if det_scale > 1:
            self._pack_rows_scaled(current_stream(), self.B, H, W, self.H, self.W, ptr(frames), ptr(self.x_in), self.x_cs)
        else:
            self._pack_rows(current_stream(), self.B, H, W, ptr(frames), ptr(self.x_in), self.x_cs)

    def run_ops(self):
        s = current_stream()
        for op in self.ops:
            if op[0] == "convs":
                op[1].run()
            elif op[0] == "pool":
                _, a, d = op
                self._maxpool(s, a.N, a.H, a.W, a.C, a.ptr, a.cs, d.ptr, d.cs)
            elif op[0] == "l2norm":
                _, a, w, d = op
                self._l2norm(s, a.N * a.H * a.W, a.C, a.ptr, a.cs, ptr(w.detach()), d.ptr, d.cs)
            else:
                _, head, a, stride, out = op
                head.decode(a, stride, out)

    def run(self):
        """every launch of the graph; returns the dense tables, one float32 [B, FH*FW, 5] per level"""
        self.run_ops()
        s = current_stream()
        for (conf, loc, ncls, stride), out in zip(self.levels, self.dense):      # fp32: the bf16 heads wrote the tables themselves
            check(self.lib.w2l_s3fd_decode(s, self.B, conf.H, conf.W, stride, conf.ptr, conf.cs, ncls, loc.ptr, loc.cs,
                                           ptr(out)), "s3fd_decode")
        return self.dense

    def dispatch(self):
        """[(layer, family, tile, ksplit)] of every bf16-storage convolution (bf16.plan_dispatch): the convb kernel each one runs"""
        return [d for p in self.plans for d in bf16.plan_dispatch(p)]

    def resolved(self):
        """[(layer, kernel family)] of every launch of `run_ops` in order: the plans' Plan.resolved() families and the glue launches
        (pool1..pool5, the L2Norm modules, the fused heads named by their feature)"""
        fams, npool, norms, heads = [], 0, iter(n for _, n, _ in HEADS if n), iter(HEADS)
        for op in self.ops:
            if op[0] == "convs":
                fams += [(name, fam) for name, _, fam, _ in op[1].resolved()]
            elif op[0] == "pool":
                npool += 1
                fams.append(("pool%d" % npool, "maxpool2x2" + self.st.suffix))
            elif op[0] == "l2norm":
                fams.append((next(norms), "l2norm_scale" + self.st.suffix))
            else:
                feat, norm, _ = next(heads)
                fams.append(("%s_mbox" % (norm or feat), "s3fd_headb"))
        return fams


class s3fd(nn.Module):
    def __init__(self):
        super().__init__()
        for item in BACKBONE:
            if not isinstance(item, str):
                name, cin, cout, k, st, p = item
                setattr(self, name, nn.Conv2d(cin, cout, kernel_size=k, stride=st, padding=p))
        self.conv3_3_norm = L2Norm(256, scale=10)
        self.conv4_3_norm = L2Norm(512, scale=8)
        self.conv5_3_norm = L2Norm(512, scale=5)
        cins = {"conv3_3": 256, "conv4_3": 512, "conv5_3": 512, "fc7": 1024, "conv6_2": 512, "conv7_2": 256}
        for feat, norm, ncls in HEADS:
            prefix = norm or feat
            setattr(self, prefix + "_mbox_conf", nn.Conv2d(cins[feat], ncls, kernel_size=3, stride=1, padding=1))
            setattr(self, prefix + "_mbox_loc", nn.Conv2d(cins[feat], 4, kernel_size=3, stride=1, padding=1))
        self._layers = {}       # the fp32 layers, (conv, activation) -> engine.FusedConv: shared by the graphs of one weight version
        self._graphs = {}
        self._version = None

    def _graph(self, B, H, W, device, precision="f32"):
        ver = engine.param_version(self)
        if ver != self._version:
            self._layers, self._graphs, self._version = {}, {}, ver
        key = (B, H, W, str(device), precision)
        g = self._graphs.get(key)
        if g is None:
            g = _Graph(self, B, H, W, torch.device(device), precision)
            self._graphs = {key: g}        # one live geometry: VGG activations of a video frame batch are large
        return g

    def forward(self, x):
        """x: float NCHW (already mean-subtracted RGB) -> [cls1, reg1, ..., cls6, reg6] NCHW, cls1 with the background
        max-out applied (net_s3fd.py:68-129)"""
        engine.require_cuda(x, "input")
        x = x.contiguous().float()
        B, Cn, H, W = x.shape
        g = self._graph(B, H, W, x.device)
        lib = load()
        s = current_stream()
        check(lib.w2l_nchw_to_nhwc(s, B, Cn, H, W, ptr(x), ptr(g.x_in), 4, 4), "nchw_to_nhwc")
        g.run_ops()
        outs = []
        for conf, loc, ncls, _ in g.levels:
            for a in (conf, loc):
                y = torch.empty((B, a.C, a.H, a.W), device=x.device, dtype=torch.float32)
                check(lib.w2l_nhwc_to_nchw(s, B, a.C, a.H, a.W, a.ptr, a.cs, ptr(y)), "nhwc_to_nchw")
                outs.append(y)
        chunk = torch.chunk(outs[0], 4, 1)          # max-out background label (3 of the 4 conf channels of level 1)
        outs[0] = torch.cat([torch.max(torch.max(chunk[0], chunk[1]), chunk[2]), chunk[3]], dim=1)
        return outs

    def dense_boxes(self, images_bgr_u8, precision="f32", det_scale=1):
        """images: torch uint8 [B,H,W,3] BGR on the device -> per level torch float32 [B, FH*FW, 5] (x1,y1,x2,y2,score):
        api.py:62 (BGR->RGB) + detect.py:57-84 for every position.  `precision`: "f32" (default) or "bf16" (the opt-in
        bf16-storage graph; a batch whose buffers would reach 2 GiB raises RuntimeError before anything is allocated).
        `det_scale` k > 1: the graph of (H // k, W // k) on the frames resized as cv2.resize does (`dense_boxes_rows` over an
        address table of the batch); the tables are in the reduced frame's coordinates."""
        engine.check_precision(precision)
        det_scale = check_det_scale(det_scale)
        if images_bgr_u8.dtype != torch.uint8 or images_bgr_u8.dim() != 4 or images_bgr_u8.shape[3] != 3:
            raise RuntimeError("dense_boxes: images must be uint8 [B,H,W,3]")
        if det_scale > 1:
            det_size(*images_bgr_u8.shape[1:3], det_scale)            # ValueError before the device is touched
        engine.require_cuda(images_bgr_u8, "images")
        img = images_bgr_u8.contiguous()
        B, H, W = img.shape[:3]
        if det_scale > 1:
            frames = torch.arange(B, dtype=torch.int64, device=img.device) * (H * W * 3) + img.data_ptr()
            return self.dense_boxes_rows(frames, B, H, W, precision, det_scale)
        g = self._graph(B, H, W, img.device, precision)
        g.pack(img)
        return g.run()

    def dense_boxes_rows(self, frames, B, H, W, precision="f32", det_scale=1):
        """`dense_boxes` for B frames named by a device address table: `frames` is a device tensor holding B uint64 addresses, each
        of pixel (0,0) of a uint8 [H,W,3] BGR frame in device memory at any byte alignment (`w2l_s3fd_pack_rows`); the frames of a
        batch need not be neighbours, nor of one clip.  Same graph, same launches and the same tables as `dense_boxes` on the
        gathered frames.  `det_scale` k > 1: the graph is the one of (B, H // k, W // k) and `w2l_s3fd_pack_rows_scaled` fills its
        input from the full-size frames."""
        engine.check_precision(precision)
        Hd, Wd = det_size(H, W, det_scale)
        engine.require_cuda(frames, "frame address table")
        if frames.numel() * frames.element_size() < 8 * B or frames.data_ptr() % 8:
            raise RuntimeError("dense_boxes_rows: the table must hold %d 8-byte aligned addresses" % B)
        g = self._graph(B, Hd, Wd, frames.device, precision)
        g.pack_rows(frames, H, W, det_scale)
        return g.run()


def nms_batch(table, gate, thresh, host_overflow=True):
    """sfd_detector.py:39-45 + bbox.py:44-64 on the device for a batch: table = torch float32 [B, P, 5] (x1, y1, x2, y2, score)
    on the HIP device; per image the rows with score > gate compete (`w2l_s3fd_nms`).  Returns (keep int32 [B, P], counts int32
    [B]): keep[b, :counts[b]] are the kept row indices of image b, best score first.

    `host_overflow=False` leaves out the one host read of `counts` and the host pass it may start: an image whose survivors of
    the gate overflowed the device pass keeps counts = -1, which `w2l_s3fd_first_rect` flags RECT_HOST - the caller decides that
    image later (face_detection/many.py re-runs its clip), and nothing waits for the device here."""
    engine.require_cuda(table, "box table")
    if table.dtype != torch.float32 or table.dim() != 3 or table.shape[2] != 5:
        raise RuntimeError("nms_batch: table must be float32 [B, P, 5]")
    table = table.contiguous()
    B, P = table.shape[:2]
    keep = torch.empty((B, P), device=table.device, dtype=torch.int32)
    counts = torch.empty((B,), device=table.device, dtype=torch.int32)
    scratch = torch.empty((B * P * 12 + 8,), device=table.device, dtype=torch.uint8)
    check(load().w2l_s3fd_nms(current_stream(), B, P, ptr(table), float(gate), float(thresh), ptr(keep), ptr(counts),
                              ptr(scratch), scratch.numel()), "s3fd_nms")
    if not host_overflow:
        return keep, counts
    over = (counts < 0).nonzero().flatten().tolist()
    for b in over:
        # more rows above the gate than the device pass holds (> 262 144: a multi-megapixel frame with a permissive gate): this
        # image's survivors go through the same greedy pass on the host - any table size works, as in the reference
        rows = (table[b, :, 4] > gate).nonzero().flatten()
        kept = _nms_host(table[b].index_select(0, rows).cpu().numpy(), thresh)
        idx = rows[torch.as_tensor(kept, dtype=torch.long, device=rows.device)].to(torch.int32)
        keep[b, :len(kept)] = idx
        counts[b] = len(kept)
    return keep, counts


RECT_NONE, RECT_FOUND, RECT_HOST = 0, 1, 2       # w2l_s3fd_first_rect flags


def first_rects(table, keep, counts, thresh, scale=None):
    """sfd_detector.py:45 + api.py:61-77 for a batch on the device (`w2l_s3fd_first_rect`): nms_batch's (keep, counts) over `table`
    -> numpy int32 [B, 5] in ONE device-to-host copy, per image (x1, y1, x2, y2, flag): the first kept row above `thresh`, clipped
    at 0 and truncated, with flag RECT_FOUND; RECT_NONE when no row passes; RECT_HOST when a coordinate is one the device does not
    convert (NaN, +inf, >= 2^31) - the caller decides that image on the host.  `scale` = (sx, sy) (`det_rect_scale`): the row is
    mapped back to the full frame first (`w2l_s3fd_first_rect_scaled`); None is the plain launch."""
    engine.require_cuda(table, "box table")
    if table.dtype != torch.float32 or table.dim() != 3 or table.shape[2] != 5:
        raise RuntimeError("first_rects: table must be float32 [B, P, 5]")
    table = table.contiguous()
    B, P = table.shape[:2]
    if keep.dtype != torch.int32 or tuple(keep.shape) != (B, P) or counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
        raise RuntimeError("first_rects: keep must be int32 [B, P] and counts int32 [B] (nms_batch's outputs)")
    keep, counts = keep.contiguous(), counts.contiguous()
    out = torch.empty((5 * B,), device=table.device, dtype=torch.int32)       # rects [B][4], then flags [B]: one copy back
    if scale is None:
        check(load().w2l_s3fd_first_rect(current_stream(), B, P, ptr(table), ptr(keep), ptr(counts), float(thresh), ptr(out),
                                         ptr(out[4 * B:])), "s3fd_first_rect")
    else:
        check(load().w2l_s3fd_first_rect_scaled(current_stream(), B, P, ptr(table), ptr(keep), ptr(counts), float(thresh),
                                                float(scale[0]), float(scale[1]), ptr(out), ptr(out[4 * B:])),
              "s3fd_first_rect_scaled")
    h = out.cpu().numpy()
    return np.concatenate([h[:4 * B].reshape(B, 4), h[4 * B:].reshape(B, 1)], axis=1)


def top_rects(table, keep, counts, thresh, K, scale=None):
    """the candidates of every image of a batch on the device (`w2l_s3fd_top_rects`, tracked face selection): `first_rects`'
    arguments and K in 1..16 -> numpy int32 (cands [B, K, 4], ncand [B], flags [B]) in ONE device-to-host copy: the first K kept
    rows above `thresh`, each converted as `first_rects` converts its one; RECT_HOST also for a coordinate above 32767."""
    engine.require_cuda(table, "box table")
    if table.dtype != torch.float32 or table.dim() != 3 or table.shape[2] != 5:
        raise RuntimeError("top_rects: table must be float32 [B, P, 5]")
    table = table.contiguous()
    B, P = table.shape[:2]
    if keep.dtype != torch.int32 or tuple(keep.shape) != (B, P) or counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
        raise RuntimeError("top_rects: keep must be int32 [B, P] and counts int32 [B] (nms_batch's outputs)")
    keep, counts = keep.contiguous(), counts.contiguous()
    K = int(K)
    n = 4 * K * B
    out = torch.empty((n + 2 * B,), device=table.device, dtype=torch.int32)   # cands [B][K][4], ncand [B], flags [B]: one copy back
    sx, sy = (1.0, 1.0) if scale is None else (float(scale[0]), float(scale[1]))
    check(load().w2l_s3fd_top_rects(current_stream(), B, P, ptr(table), ptr(keep), ptr(counts), float(thresh), sx, sy, K, ptr(out),
                                    ptr(out[n:]), ptr(out[n + B:])), "s3fd_top_rects")
    h = out.cpu().numpy()
    return h[:n].reshape(B, K, 4), h[n:n + B], h[n + B:]


def _nms_host(dets, thresh):
    """bbox.py:44-64 in its float32 operation order (numpy): kept row indices of `dets` [n, 5], best score first.  Only the
    overflow route of nms_batch comes here."""
    d = np.asarray(dets, dtype=np.float32)
    x1, y1, x2, y2, sc = (d[:, i] for i in range(5))
    one = np.float32(1)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.lexsort((np.arange(len(d)), sc))[::-1]        # score descending, equal scores: the later row first (as the device pass)
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        rest = order[1:]
        w = np.maximum(np.float32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + one)
        h = np.maximum(np.float32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + one)
        inter = w * h
        ovr = inter / (areas[i] + areas[rest] - inter)
        order = rest[ovr <= np.float32(thresh)]
    return keep


def nms(dets, thresh):
    """`nms(dets, thresh)` of bbox.py:44-64: dets [n, 5] (numpy or torch) -> list of kept row indices, best score first.
    Runs on the HIP device (every row competes: the gate is -inf)."""
    if 0 == len(dets):
        return []
    t = torch.as_tensor(np.ascontiguousarray(dets) if isinstance(dets, np.ndarray) else dets, dtype=torch.float32)
    keep, counts = nms_batch(t.to("cuda").reshape(1, -1, 5), float("-inf"), thresh)
    return keep[0, :int(counts[0].item())].cpu().tolist()
