"""`SyncNet_color`, the expert lip-sync discriminator, with the reference's API and state-dict keys
(models/syncnet.py:7-66): face (B,15,48,96) and mel (B,1,80,16) -> two L2-normalised 512-d embeddings."""
import torch
from torch import nn

from .. import autograd, bf16, engine
from .._lib import check, current_stream, load, ptr
from .wav2lip import _down, _res, audio_encoder_rows, check_precision, make_stack

SYNC_FACE_ENCODER = (                              # models/syncnet.py:11-33
    [("c", 15, 32, 7, 1, 3, 0),
     ("c", 32, 64, 5, (1, 2), 1, 0)] + _res(64, 2)
    + _down(64, 128, 3) + _down(128, 256, 2) + _down(256, 512, 2)
    + [("c", 512, 512, 3, 2, 1, 0), ("c", 512, 512, 3, 1, 0, 0), ("c", 512, 512, 1, 1, 0, 0)])


def bf16_buffer_sizes(N, H=48, W=96):
    """bytes of every buffer the bf16 _SyncGraph allocates for batch N and an H x W face input, from the layer tables alone: the two bf16
    inputs (16 and 8 channels), then every layer's bf16 output"""
    sizes = [2 * N * H * W * 16, 2 * N * 80 * 16 * 8]
    for rows, (h, w) in ((SYNC_FACE_ENCODER, (H, W)), (audio_encoder_rows(2), (80, 16))):
        for _, _, cout, k, s, p, _ in rows:
            sh, sw = engine._pair(s)
            h, w = (h + 2 * p - k) // sh + 1, (w + 2 * p - k) // sw + 1
            if h < 1 or w < 1:
                raise RuntimeError("input too small for the SyncNet encoders")
            sizes.append(2 * N * h * w * bf16.round8(cout))
    return sizes


def bf16_batch_limit(H=48, W=96):
    """the first batch size at which a buffer of the bf16 _SyncGraph reaches 2 GiB (every size is linear in N)"""
    return -(-bf16.BUF_LIMIT // max(bf16_buffer_sizes(1, H, W)))


def check_bf16_buffers(N, H=48, W=96):
    big = max(bf16_buffer_sizes(N, H, W))
    if big >= bf16.BUF_LIMIT:
        raise RuntimeError("SyncNet bf16: a batch of %d windows (%d x %d) needs a %d-byte buffer, over the kernels' 2 GiB limit: "
                           "batches below %d fit" % (N, H, W, big, bf16_batch_limit(H, W)))


class _SyncGraph:
    """The inference plan of both encoders for one (batch, height, width, device) in one storage (engine.storage): "f32", or "bf16",
    the opt-in bf16-STORAGE plan - bf16 NHWC inputs (15 + 1 and 1 + 7 channels), every layer a bf16.ConvB launch with its eval-mode
    BatchNorm folded into the fp32 epilogue, the two 512-channel outputs stored in bf16 like every other layer.  `embeddings`
    normalises the two outputs into fp32."""

    def __init__(self, model, N, H, W, device, precision="f32"):
        st = self.st = engine.storage(precision)
        self.precision = st.name
        if st is engine.BF16:
            check_bf16_buffers(N, H, W)        # before anything is allocated
        self.lib = lib = load()
        self.N, self.H, self.W = N, H, W
        pool = engine.BufPool(device, st)
        plan = engine.Plan()
        self.face_in = st.new_buf(N, H, W, 16, device, zero=True)      # 15 channels + 1 zero pad
        self.mel_in = st.new_buf(N, 80, 16, 4, device, zero=True)      # 1 mel channel + zero pad: 4 channels in fp32, 8 in bf16
        self.face_cs, self.mel_cs = self.face_in.shape[3], self.mel_in.shape[3]
        self.face_out, _ = engine.run_chain(plan, pool, "face_encoder", list(model.face_encoder), st.act(self.face_in, 0, 15))
        self.audio_out, _ = engine.run_chain(plan, pool, "audio_encoder", list(model.audio_encoder), st.act(self.mel_in, 0, 1))
        for o in (self.face_out, self.audio_out):
            if (o.H, o.W) != (1, 1):
                raise RuntimeError("SyncNet encoders must end at 1x1, got %dx%d" % (o.H, o.W))
        plan.tuned = st.shape_tuned
        self.plan = plan
        self.scratch_bytes = pool.total_bytes
        self._to_nhwc, self._window_rows = st.bind(lib, "nchw_to_nhwc"), st.bind(lib, "sync_window_rows")

    def dispatch(self, N=None):
        """[(record name, family, tile, ksplit)] of every bf16-storage launch of the plan (bf16.plan_dispatch): the kernel each one
        runs, or would run at batch N"""
        return bf16.plan_dispatch(self.plan, N)

    def load_nchw(self, audio, face):
        """contiguous fp32 [N,1,80,16] and [N,C,H,W] device tensors -> the plan's two inputs"""
        s, fc, mc = current_stream(), self.face_cs, self.mel_cs
        self._to_nhwc(s, self.N, face.shape[1], self.H, self.W, ptr(face), ptr(self.face_in), fc, fc)
        self._to_nhwc(s, self.N, 1, 80, 16, ptr(audio), ptr(self.mel_in), mc, mc)

    def load_rows(self, rows, B):
        """the plan's two inputs from B w2l_sync_row entries (96x96 face crops)"""
        self._window_rows(current_stream(), B, ptr(rows), 96, ptr(self.face_in), self.face_cs, ptr(self.mel_in), self.mel_cs)

    def embeddings(self, B, audio_ptr, face_ptr):
        """the plan's two outputs, L2-normalised, into fp32 [B, 512] rows at the two addresses: two w2l_l2norm_rows launches in
        fp32, one w2l_sync_embeddings_bf16 launch in bf16"""
        s, a, v = current_stream(), self.audio_out, self.face_out
        if self.st is engine.BF16:
            check(self.lib.w2l_sync_embeddings_bf16(s, B, 512, a.ptr, a.cs, v.ptr, v.cs, audio_ptr, face_ptr), "sync_embeddings_bf16")
        else:
            check(self.lib.w2l_l2norm_rows(s, B, 512, a.ptr, a.cs, audio_ptr), "l2norm_rows")
            check(self.lib.w2l_l2norm_rows(s, B, 512, v.ptr, v.cs, face_ptr), "l2norm_rows")


class SyncNet_color(nn.Module):
    def __init__(self):
        super().__init__()
        self.face_encoder = make_stack(SYNC_FACE_ENCODER)
        self.audio_encoder = make_stack(audio_encoder_rows(2))
        self._graphs = {}
        object.__setattr__(self, "_train_graphs", autograd.GraphCache(autograd.build_syncnet))

    def forward(self, audio_sequences, face_sequences, precision="f32"):
        """`precision` "bf16" (inference only): the opt-in bf16-storage plan; the embeddings stay fp32"""
        check_precision(precision)
        engine.require_cuda(face_sequences, "face_sequences")
        with engine.on_device_of(face_sequences, self):      # launches go to the current stream of the INPUT's device; refuses a device mismatch
            return self._forward_impl(audio_sequences, face_sequences, precision)

    def _forward_impl(self, audio_sequences, face_sequences, precision="f32"):
        engine.require_cuda(face_sequences, "face_sequences")
        engine.require_cuda(audio_sequences, "audio_sequences")
        face = face_sequences.contiguous().float()
        audio = audio_sequences.contiguous().float()
        N, C_, H, W = face.shape
        if autograd.needs_graph(self, (audio, face)):
            if precision != "f32":
                raise ValueError("SyncNet_color: precision=%r is an inference switch (eval mode, no gradients); training precision "
                                 "is engine.set_train_precision" % (precision,))
            # train mode (color_syncnet_train.py:150-158) or the frozen expert inside the generator's loss
            # (wav2lip_train.py:187-198, which never calls .eval(): BN runs on batch statistics there too)
            a, v = autograd.run_graph(self._train_graphs, self, (N, H, W, str(face.device)), (N, H, W, face.device),
                                      (audio, face))
            return autograd.L2NormRows.apply(a.reshape(N, -1)), autograd.L2NormRows.apply(v.reshape(N, -1))
        g = self._eval_graph(N, H, W, face.device, precision)
        g.load_nchw(audio, face)
        g.plan.run()
        a = torch.empty((N, 512), device=face.device, dtype=torch.float32)
        v = torch.empty((N, 512), device=face.device, dtype=torch.float32)
        g.embeddings(N, ptr(a), ptr(v))
        return a, v

    def _eval_graph(self, N, H, W, device, precision="f32"):
        """the one cached inference graph: another (N, H, W), device, precision or weight version replaces it"""
        ver = engine.param_version(self)
        key = (N, H, W, str(device), precision)
        g = self._graphs.get(key)
        if g is None or g[0] != ver:
            self._graphs.clear()
            g = (ver, _SyncGraph(self, N, H, W, device, precision))
            self._graphs[key] = g
        return g[1]

    def embed_rows(self, rows, B, audio_out, face_out, offset=0, precision="f32"):
        """Eval mode only: the embeddings of the `B` windows of a device row table (w2l_sync_row, include/w2l_hip.h; 96x96 face
        crops) into audio_out[offset:offset+B] and face_out[offset:offset+B], two contiguous fp32 [rows, 512] device tensors.
        w2l_sync_window_rows writes the graph's two inputs from the table, the plan runs, w2l_l2norm_rows writes the outputs:
        no tensor is made on the way.  The graph cache is `forward`'s: a caller that keeps to one `B` builds one plan.
        `precision` "bf16": w2l_sync_window_rows_bf16, the bf16-storage plan, w2l_sync_embeddings_bf16; the outputs stay fp32."""
        check_precision(precision)
        if self.training:
            raise RuntimeError("SyncNet_color.embed_rows is an inference path: call .eval() first")
        engine.require_cuda(face_out, "face_out")
        for name, t in (("audio_out", audio_out), ("face_out", face_out)):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 512 or not t.is_contiguous() or t.device != face_out.device:
                raise ValueError("%s must be a contiguous fp32 [rows, 512] tensor on %s" % (name, face_out.device))
            if not 0 <= offset <= t.shape[0] - B:
                raise ValueError("rows [%d, %d) are outside the %d rows of %s" % (offset, offset + B, t.shape[0], name))
        if rows.device != face_out.device or rows.dtype != torch.uint8 or not rows.is_contiguous() or rows.numel() < 32 * B or B < 1:
            raise ValueError("rows must be a contiguous uint8 device tensor holding B >= 1 w2l_sync_row entries")
        with engine.on_device_of(face_out, self):
            g = self._eval_graph(B, 48, 96, face_out.device, precision)
            g.load_rows(rows, B)
            g.plan.run()
            g.embeddings(B, audio_out.data_ptr() + 2048 * offset, face_out.data_ptr() + 2048 * offset)
