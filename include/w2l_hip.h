/*
 * w2l_hip.h — C ABI of libw2l_hip.so: the MI355X (gfx950) kernels behind the Wav2Lip hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes and a HIP stream
 * (passed as `void*`, i.e. a `hipStream_t`; NULL = the null stream), enqueues work on that
 * stream and returns without synchronising.  Return value: 0 = ok, negative = error; the
 * message of the last error on the calling thread is returned by w2l_last_error().
 * Nothing is thrown across the ABI.  Caller owns every tensor; the library owns only the
 * handles it creates (packed weights, tap tables, plans) and frees them in *_destroy.
 *
 * Activation layout is NHWC fp32 with an explicit per-pixel channel stride ("cs", in floats):
 * a tensor argument is (pointer to channel 0 of pixel 0, cs).  That is how the skip-concats
 * of the generator (reference models/wav2lip.py:104-114) disappear: producers write straight
 * into channel slices of the concat buffer.
 *
 * Reference interfaces replaced (paths relative to the Rudrabha/Wav2Lip checkout):
 *   w2l_conv_*            models/conv.py:5-19 (Conv2d = conv+BN(+res)+ReLU), :21-31 (nonorm_Conv2d),
 *                         :33-44 (Conv2dTranspose); bare conv + Sigmoid heads models/wav2lip.py:84-85,152
 *   w2l_bn_fold           the eval-mode nn.BatchNorm2d inside those blocks (models/conv.py:10,40)
 *   w2l_nchw_to_nhwc,
 *   w2l_nhwc_to_nchw      the layout glue at inference.py:259-260,265 and models/wav2lip.py:93-94,118-120
 *   w2l_datagen_pack      inference.py:133-143 (mask lower half, concat, /255.) + :259 (transpose, f64->f32)
 *   w2l_frames_to_u8      inference.py:265,269 (x255, astype(uint8) truncation, NHWC)
 *   w2l_crop_resize_u8    inference.py:121-126 (face crop -> cv2.resize to 96x96)
 *   w2l_resize_paste_u8   inference.py:270-271 (cv2.resize of the generated crop to the box size + paste into the frame)
 *   w2l_crop_resize_rows_u8  evaluation/gen_videos_from_filelist.py:85-95 (the same crop + resize, one frame per row)
 *   w2l_compose_rows_u8   evaluation/gen_videos_from_filelist.py:221-227 (resize + paste + the frame copy, one pass)
 *   w2l_resize_rows_u8    evaluation/real_videos_inference.py:51-70,239-245 (the whole-frame cv2.resize of the `max_frame_res`
 *                         cap and of rescale_frames, one frame per row)
 *   w2l_jpeg_encode_rows  preprocess.py:62 (cv2.imwrite of every face crop as <i>.jpg), one crop per row
 *   w2l_jpeg_decode_rows  wav2lip_train.py:66, color_syncnet_train.py:97 (cv2.imread of every <id>.jpg), one file per row
 *   w2l_jpeg_encode_rows_rst  inference.py:256-257,272 (cv2.VideoWriter + out.write(f): the compressed result video; here Motion-JPEG,
 *                         every frame a JPEG with restart intervals), one frame per row
 *   w2l_jpeg_decode_rows_rst  inference.py:189-215 (cv2.VideoCapture(args.face) ... video_stream.read()) for a Motion-JPEG video,
 *                         one lane per restart interval
 *   w2l_mel_gather_rows   evaluation/gen_videos_from_filelist.py:176-183 (mel windows, one spectrogram per row)
 *   w2l_s3fd_pack_rows    face_detection/api.py:62 + detection/sfd/detect.py:57-63 (the detector's input), one frame per row
 *   w2l_s3fd_pack_rows_scaled  inference.py:202-203 (the `cv2.resize(frame, (w // k, h // k))` of --resize_factor) fused into the
 *                         detector's input: detection at reduced size, output frames untouched (--face_det_scale)
 *   w2l_s3fd_first_rect_scaled  face_detection/api.py:61-77 with the rect mapped back to the full frame first
 *   w2l_s3fd_top_rects    face_detection/detection/sfd/sfd_detector.py:45 + api.py:61-77 for the first K kept boxes above 0.5, where
 *                         the reference keeps d[0] alone (opt-in: `face_track`)
 *   w2l_face_track_segments  api.py:61-77's choice of one box per frame, made over the clip instead: a face is followed from
 *                         frame to frame by overlap (opt-in, not the reference's rule: `face_track`)
 *   w2l_face_boxes_segments  evaluation/gen_videos_from_filelist.py:35-42, :61-77 = inference.py:59-66, :90-104 (pads, clipping,
 *                         "Face not detected", get_smoothened_boxes) for every clip of a group in one launch
 *   w2l_face_boxes_stream  inference.py:59-66, :90-104 for live streams: the same boxes, written tick by tick as frames arrive
 *   w2l_face_boxes_runs, w2l_face_boxes_stream_runs  the two above with frames without a face passed through (opt-in, not the
 *                         reference's: `no_face_hold`)
 *   w2l_face_spans_segments  the face tracks evaluation/scores_LSE/calculate_scores_real_videos.py scores: misses bridged by
 *                         interpolation, short tracks dropped (opt-in, not the reference's code: `track_spans`)
 *   w2l_face_tracks_all_segments  the same file's :38-40, one line per face track: every face of a shot followed at once, where
 *                         w2l_face_track_segments follows one (opt-in: `all_faces`)
 *   w2l_face_rects_expand_segments  inference.py:77-78 (the detector's loop over ALL frames) made shorter: the detector sees every
 *                         Nth frame and the rects between are interpolated (opt-in, not the reference's: `det_stride`)
 *   w2l_melspectrogram    audio.py:45-51 (preemphasis, STFT, mel basis, dB, normalise)
 *   w2l_mel_gather        inference.py:231-240 (16-frame mel windows at host-computed starts)
 *   w2l_resample_sinc     audio.py:9-10 (librosa.core.load's sample-rate conversion: resampy 'kaiser_best' sinc interpolation)
 *   w2l_resample_stream   the same conversion for live streams: the final output samples of many streams per launch
 *   w2l_l2norm_rows       models/syncnet.py:62-63 (F.normalize(p=2, dim=1))
 *   w2l_cosine_bce        wav2lip_train.py:179-184 (cosine_similarity + BCELoss)
 *   w2l_plan_*            the per-batch forward loop inference.py:262-263 -> models/wav2lip.py:87-125
 *
 * Training side (the torch autograd graph behind loss.backward() / optimizer.step() at wav2lip_train.py:229-230,
 * color_syncnet_train.py:164-165, hq_wav2lip_train.py:231-232,256-257):
 *   w2l_conv_update       re-pack a layer after an optimiser step (weights change every step)
 *   w2l_conv_wgrad        weight gradient of nn.Conv2d / nn.ConvTranspose2d (models/conv.py:8,24,36)
 *                         (the data gradient is w2l_conv_forward on the transposed geometry)
 *   w2l_bn_train_stats,
 *   w2l_affine_act,
 *   w2l_bn_train_bwd      nn.BatchNorm2d in batch-statistics mode + residual + ReLU, forward and backward
 *                         (models/conv.py:10-12,17-19,40-43)
 *   w2l_act_bwd           backward of ReLU / LeakyReLU / Sigmoid (+ eval-mode BN scale) (models/conv.py:12,27;
 *                         models/wav2lip.py:85,152)
 *   w2l_col_sum           bias gradients
 *   w2l_l1_mean/_bwd      nn.L1Loss (wav2lip_train.py:191,227)
 *   w2l_cosine_bce_bwd    backward of cosine_loss (wav2lip_train.py:179-184)
 *   w2l_l2norm_bwd        backward of F.normalize (models/syncnet.py:62-63)
 *   w2l_bce_bwd           backward of F.binary_cross_entropy (models/wav2lip.py:171, hq_wav2lip_train.py:249,253)
 *   w2l_adam_*            optim.Adam (wav2lip_train.py:359, hq_wav2lip_train.py:418-421)
 *   w2l_shifted_pdist     calc_pdist of the LSE-D / LSE-C scorer (evaluation/scores_LSE/SyncNetInstance_calc_scores.py:19-31)
 *   w2l_sync_window_rows,
 *   w2l_sync_window_rows_bf16  the scorer's window building (SyncNetInstance_calc_scores.py:105-127), one clip per row
 *   w2l_sync_embeddings_bf16  models/syncnet.py:62-63 (F.normalize(p=2, dim=1)) of both bf16 encoder outputs in one launch
 *   w2l_lse_score_segments  its scores (SyncNetInstance_calc_scores.py:19-31,129-137) for every clip of a directory run
 *                         (evaluation/scores_LSE/calculate_scores_LRS.py:28-50) in one launch
 */
#ifndef W2L_HIP_H
#define W2L_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2L_OK 0
#define W2L_ERR_ARG (-1)      /* bad argument / unsupported geometry */
#define W2L_ERR_HIP (-2)      /* a HIP runtime call failed */
#define W2L_ERR_NOMEM (-3)

/* activation applied after y = acc*scale + shift (+ residual) */
#define W2L_ACT_NONE 0
#define W2L_ACT_RELU 1        /* models/conv.py:12  */
#define W2L_ACT_SIGMOID 2     /* models/wav2lip.py:85 */
#define W2L_ACT_LEAKY 3       /* LeakyReLU(0.01), models/conv.py:27 */

/* arithmetic of a conv layer's contraction (tensors in HBM are fp32 either way) */
#define W2L_PREC_F32 0        /* exact fp32 products on the fp32 matrix cores (default; the inference parity path) */
#define W2L_PREC_BF16 1       /* operands rounded to bf16 (RNE) inside the kernel, fp32 accumulate, bf16 matrix cores:
                                 the mixed precision BASELINE configs 4/5 name for training */

const char* w2l_last_error(void);
/* library/ABI version, bumped on any signature change */
int w2l_abi_version(void);
/* number of visible HIP devices (<=0: none/err) and the gcnArchName of `dev` copied into buf */
int w2l_device_count(void);
int w2l_device_arch(int dev, char* buf, size_t buflen);

/* ---------------------------------------------------------------- fused convolution layers */

typedef struct w2l_conv_geom {
    int transposed;           /* 0: nn.Conv2d weight [cout][cin][kh][kw]; 1: nn.ConvTranspose2d weight [cin][cout][kh][kw] */
    int cin, cout;
    int kh, kw;
    int sh, sw;               /* stride */
    int ph, pw;               /* padding */
    int oph, opw;             /* output_padding (transposed only) */
    int act;                  /* W2L_ACT_* */
} w2l_conv_geom;

typedef struct w2l_conv w2l_conv_t;

/* Build a layer: packs `weight` (torch layout, device, fp32) into the kernel's K-major layout
 * (one slab per output phase for transposed convs), copies scale/shift ([cout], device).
 * y = act( conv(x, weight) * scale + shift (+ res) ).  The input buffer must provide
 * w2l_conv_cin_padded(cin) readable channels per pixel with the pad channels ZERO. */
int w2l_conv_create(const w2l_conv_geom* g, const float* weight, const float* scale,
                    const float* shift, void* stream, w2l_conv_t** out);
int w2l_conv_destroy(w2l_conv_t* c);
/* Re-pack the layer for new parameters (asynchronous on `stream`, no allocation, no synchronisation): any of
 * weight / scale / shift may be NULL = unchanged.  The caller's tensors must stay alive until the stream reaches
 * the copies (stream-ordered, as for any other kernel argument). */
int w2l_conv_update(w2l_conv_t* c, const float* weight, const float* scale, const float* shift, void* stream);
int w2l_conv_cin_padded(int cin);                       /* roundup(cin, 4) */
int w2l_conv_out_hw(const w2l_conv_geom* g, int H, int W, int* Ho, int* Wo);
/* Enqueue one fused layer.  x: [N,H,W,x_cs] fp32 (first cin_padded channels of each pixel used);
 * y: [N,Ho,Wo,y_cs] (first cout channels of each pixel written); res: optional [N,Ho,Wo,res_cs]
 * residual added before the activation (NULL = none).  res may alias x. */
int w2l_conv_forward(const w2l_conv_t* c, void* stream, int N, int H, int W,
                     const float* x, int x_cs, float* y, int y_cs,
                     const float* res, int res_cs);
/* Fuse a following 1x1 convolution + activation into the layer's epilogue (the generator's RGB head, reference
 * models/wav2lip.py:83-85: Conv2d(80,32,3)+BN+ReLU -> nn.Conv2d(32,head_c,1) -> Sigmoid): after this call w2l_conv_forward
 * writes y[pix][o] = head_act( sum_c head_weight[o][c] * act(...)[c] + head_bias[o] ), o < head_c <= 4, instead of the cout
 * channels (which never reach HBM).  head_weight [head_c][cout], head_bias [head_c] or NULL: device fp32.  Needs
 * cout % 4 == 0 and cout <= 128; residual inputs are not supported on a layer with a head. */
int w2l_conv_attach_head(w2l_conv_t* c, const float* head_weight, const float* head_bias, int head_c, int head_act,
                         void* stream);
/* nominal multiply-accumulates of one forward at (N,H,W) — the reference's direct-conv count */
long long w2l_conv_macs(const w2l_conv_geom* g, int N, int H, int W);
/* select the contraction arithmetic of this layer (W2L_PREC_*); Winograd is only used with W2L_PREC_F32 */
int w2l_conv_set_precision(w2l_conv_t* c, int precision);
/* tile configuration override for tuning/tests: -1 = automatic */
int w2l_conv_set_tile(w2l_conv_t* c, int tile_id);
int w2l_conv_num_tiles(void);

/* scale = gamma/sqrt(var+eps); shift = (bias-mean)*scale + beta.  Any of bias/gamma/beta/mean/var may
 * be NULL (treated as 0 / 1 / 0 / 0 / 1 with eps ignored when var is NULL): covers conv+BN (models/conv.py:8-11),
 * bare conv with bias (models/wav2lip.py:84) and nonorm conv (models/conv.py:24-26). */
int w2l_bn_fold(void* stream, int C, const float* bias, const float* gamma, const float* beta,
                const float* mean, const float* var, float eps, float* scale, float* shift);

/* ---------------------------------------------------------------- layout / data path */

/* x [N,C,H,W] fp32 -> y [N,H,W,y_cs] channels [0,C); channels [C,c_zero_to) of each pixel are zero-filled */
int w2l_nchw_to_nhwc(void* stream, int N, int C, int H, int W, const float* x, float* y, int y_cs,
                     int c_zero_to);
/* x [N,H,W,x_cs] (first C channels) -> y [N,C,H,W] */
int w2l_nhwc_to_nchw(void* stream, int N, int C, int H, int W, const float* x, int x_cs, float* y);

/* faces u8 [N,S,S,3] (BGR crops already SxS) -> x fp32 [N,S,S,y_cs]:
 * ch0-2 = face with rows >= S/2 zeroed, ch3-5 = face, all (float)((double)v/255.0); ch6..c_zero_to-1 = 0.
 * inference.py:136-139,259 */
int w2l_datagen_pack(void* stream, int N, int S, const uint8_t* faces, float* y, int y_cs, int c_zero_to);
/* the same packing into bf16 [N,S,S,y_cs] for the bf16-storage generator: each fp32 value above rounded once (RNE) */
int w2l_datagen_pack_bf16(void* stream, int N, int S, const uint8_t* faces, void* y, int y_cs, int c_zero_to);
/* pred fp32 [N,H,W,x_cs] (first 3 ch, values in [0,1]) -> u8 [N,H,W,3] = (uint8)(v*255.f) (truncation).
 * inference.py:265,269 */
int w2l_frames_to_u8(void* stream, int N, int H, int W, const float* x, int x_cs, uint8_t* y);

/* Box tensors below: int32 [B][4] = (y1, y2, x1, x2) per item, device memory, 16-byte aligned, 0 <= y1 < y2 <= H and
 * 0 <= x1 < x2 <= W; frame_idx int32 [B] selects the frame of each item (NULL = item b uses frame b).  Resizing follows
 * cv::resize(INTER_LINEAR) for CV_8UC3 (OpenCV 4.1.0 fixed-point path, see csrc/resize.hip).
 *
 * PRECONDITION of the five image entry points (w2l_crop_resize_u8, w2l_resize_u8, w2l_resize_paste_u8, w2l_crop_resize_rows_u8,
 * w2l_compose_rows_u8) and of the two blend forms (w2l_resize_blend_u8, w2l_compose_blend_rows_u8): every box is non-empty and inside its frame, and every frame_idx names an existing frame.  The boxes
 * live in device memory, so the entry points cannot look at them and the kernels do not: an empty or inverted box makes the tap
 * clamp of a source size <= 0 read index -1, and two negative extents give the paste a positive pixel count.  The HOST caller
 * checks them before the launch (wav2lip_amd/inference.py validate_boxes, and what multiclip, streaming, calculate_scores and
 * data build on it).  What the entry points do check and refuse with an error code, writing nothing: NULL pointers, B outside
 * [1, 65535], sizes below 1, a box or row table that is not 16-byte aligned. */

/* out u8 [B,S,S,3] = resize(frames[frame_idx[b]][y1:y2, x1:x2], (S,S)):  inference.py:121-126 */
int w2l_crop_resize_u8(void* stream, int B, const uint8_t* frames, int H, int W, const int32_t* frame_idx,
                       const int32_t* boxes, int S, uint8_t* out);
/* dst u8 [B,Hd,Wd,3] = resize(src u8 [B,Hs,Ws,3], (Wd, Hd)): the `--resize_factor` step of inference.py:202-203 */
int w2l_resize_u8(void* stream, int B, const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd);
/* frames[frame_idx[b]][y1:y2, x1:x2] = resize(pred[b] (u8 [S,S,3]), (x2-x1, y2-y1)), in place:  inference.py:270-271.
 * max_box_pixels >= the largest (y2-y1)*(x2-x1) of the batch (sizes the launch). */
int w2l_resize_paste_u8(void* stream, int B, const uint8_t* pred, int S, const int32_t* boxes, const int32_t* frame_idx,
                        uint8_t* frames, int H, int W, int max_box_pixels);

/* Row-table forms (evaluation/gen_videos_from_filelist.py:85-95 crop + cv2.resize of every row's face, :221-227 cv2.resize of
 * the generated crop + paste + out.write of the WHOLE frame): a row is one generator input and names its own frame, so rows
 * of clips with different frame shapes share one launch.  Tables live in device memory, 16-byte aligned.
 *
 * w2l_frame_row, 48 bytes, alignment 16:
 *   offset  0  uint64 src    device address of pixel (0,0) of the row's source frame, u8 [H,W,3] BGR
 *   offset  8  uint64 dst    device address of the row's output frame u8 [H,W,3] (compose only; src == dst: paste in place)
 *   offset 16  int32  H, W   that frame's size (differs from row to row)
 *   offset 24  int32  y1, y2, x1, x2   face box, 0 <= y1 < y2 <= H, 0 <= x1 < x2 <= W (validated by the caller)
 *   offset 40  int32  pad[2] unused (keeps consecutive rows 16-byte aligned)
 * w2l_mel_row, 16 bytes, alignment 16:
 *   offset  0  uint64 mel    device address of the row's spectrogram, fp32 [80][T]
 *   offset  8  int32  T      its number of columns
 *   offset 12  int32  start  the window is columns [start, start+16) (columns outside [0,T) read as 0) */
typedef struct {
    uint64_t src, dst;
    int32_t H, W;
    int32_t y1, y2, x1, x2;
    int32_t pad[2];
} w2l_frame_row;
typedef struct {
    uint64_t mel;
    int32_t T, start;
} w2l_mel_row;

/* out u8 [B,S,S,3]: out[b] = resize(frame_b[y1:y2, x1:x2], (S,S)); byte-equal to w2l_crop_resize_u8 */
int w2l_crop_resize_rows_u8(void* stream, int B, const w2l_frame_row* rows, int S, uint8_t* out);
/* dst_b = src_b outside the box, resize(pred[b] (u8 [S,S,3]), (x2-x1, y2-y1)) inside it: ONE pass writes the whole output frame
 * (byte-equal to a frame copy + w2l_resize_paste_u8).  src == dst: paste in place.  max_frame_pixels >= the largest H*W of
 * the batch (sizes the launch). */
int w2l_compose_rows_u8(void* stream, int B, const uint8_t* pred, int S, const w2l_frame_row* rows, int max_frame_pixels);

/* Feathered, mouth-region forms of the two pastes (opt-in: NOT the reference's output, which is the hard rectangle above).
 * Integer-only and exact.  Per box of h x w pixels, with feather F in [0, 64] (pixels of the output frame) and top_q8 T in
 * [0, 255] (T = 128 keeps the original upper half of the box), box-relative row j and column i:
 *   t0 = (h*T) >> 8;  hr = h - t0 (>= 1);  Fe = min(F, (min(w, hr) - 1) / 2);  D = (Fe+1)^2
 *   wy(j) = 0 for j < t0, else min(Fe+1, j-t0+1, h-j);  wx(i) = min(Fe+1, i+1, w-i);  a = wx*wy
 *   out_c = (a*p_c + (D-a)*o_c + D/2) / D      (floor; at most 4225*255 + 2112, 32-bit)
 * p = the pixel the plain paste writes (the same copy / 2x area / 11-bit bilinear resize), o = the frame's own pixel.  Fe is per
 * box, so the centre of a small box still reaches a == D.  F = 0, T = 0: a == D == 1, byte-equal to the plain paste.  Pixels with
 * a == 0 are never resized: copied from the source, or skipped in place.
 *
 * w2l_resize_blend_u8: in place, as w2l_resize_paste_u8 (one thread reads and writes a pixel); same preconditions and argument
 * checks.  Two items that name one destination frame are undefined, as there.
 * w2l_compose_blend_rows_u8: as w2l_compose_rows_u8; o is read from src, dst is written, src == dst blends in place.
 * Both refuse feather outside [0, 64] and top_q8 outside [0, 255] with an error code, writing nothing. */
int w2l_resize_blend_u8(void* stream, int B, const uint8_t* pred, int S, const int32_t* boxes, const int32_t* frame_idx,
                        uint8_t* frames, int H, int W, int max_box_pixels, int feather, int top_q8);
int w2l_compose_blend_rows_u8(void* stream, int B, const uint8_t* pred, int S, const w2l_frame_row* rows, int max_frame_pixels,
                              int feather, int top_q8);

/* Colour matching of generated faces to the crops they were generated from (opt-in: NOT the reference's output, which pastes
 * the prediction as the generator gave it).  Integer-only and exact.  Row b: pred u8 [S,S,3] (the generator's output) and ref
 * u8 [S,S,3] (the crop it was given), both BGR, rows contiguous.  The generator is shown the upper half of the crop unmasked,
 * so the statistics are taken over rows 0 .. S/2-1 only (N = S/2 * S pixels), per channel:
 *   Sp = sum pred, So = sum ref, Qp = sum pred^2, Qo = sum ref^2         (exact, uint32 for S <= 256)
 *   Vp = N*Qp - Sp^2, Vo = N*Qo - So^2                                    (>= 0, uint64)
 *   mode 1 (mean): g = 256
 *   mode 2 (full): g = 256 if Vp == 0, else clamp(isqrt(floor((Vo << 16) / Vp)), 128, 512)   (floor square root; Q8, [0.5, 2])
 * and every pixel x of that channel, in all S rows, becomes
 *   out = clamp(floor((g*(N*x - Sp) + 256*So + 128*N) / (256*N)), 0, 255)      (int64; floor division of a signed numerator)
 * Equal upper halves give out == pred everywhere.  The arithmetic is csrc/color_match_core.h, shared with a host program.
 *
 * out == pred is allowed (in place: a row's statistics are complete before any byte of it is written); out may otherwise not
 * overlap pred; ref is never written; nothing outside out[0 .. B*S*S*3) is written.  Any base address works.  One launch
 * whatever B; B == 0 launches nothing.  Refused with an error code, writing nothing: B < 0, S odd or outside [2, 256], mode
 * other than 1 or 2, a NULL pointer with B > 0. */
int w2l_color_match_u8(void* stream, int B, const uint8_t* pred, const uint8_t* ref, int S, int mode, uint8_t* out);

/* Whole-frame row-table resize (evaluation/real_videos_inference.py:51-70 rescale_frames, :239-245 the `max_frame_res` cap at read
 * time): row b gives dst_b u8 [Hd,Wd,3] = cv2.resize(src_b u8 [Hs,Ws,3], (Wd,Hd)), byte-equal to w2l_resize_u8 for that frame
 * (the same arithmetic, the equal-size copy and the exact-2x INTER_AREA branch included).  Rows of different shapes share one
 * launch; two rows may name one src (a duplicated frame); src and dst may lie at ANY byte address (frames of a clip are packed
 * back to back and H*W*3 is rarely a multiple of 4).  max_dst_pixels >= the largest Hd*Wd of the batch (sizes the launch),
 * at most 2^29.  The table lives in device memory, 16-byte aligned.
 *
 * w2l_resize_row, 32 bytes, alignment 16:
 *   offset  0  uint64 src    device address of pixel (0,0) of the row's source frame, u8 [Hs,Ws,3]
 *   offset  8  uint64 dst    device address of the row's destination frame, u8 [Hd,Wd,3]; no dst overlaps a src or another dst
 *   offset 16  int32  Hs, Ws, Hd, Wd   both sizes, each >= 1 (validated by the caller); consecutive rows stay 16-byte aligned
 *
 * PRECONDITION: every size of every row is at least 1 and Hd*Wd <= max_dst_pixels.  The sizes live in device memory, so the
 * entry point cannot look at them and the kernel does not: a source size <= 0 makes the tap clamp read index -1, and a
 * destination larger than max_dst_pixels <= 2^29 overflows the item count.  The HOST caller checks them before the launch
 * (wav2lip_amd/real_videos_inference.py resize_rows).  What the entry point does check and refuse with an error code, writing
 * nothing: NULL pointers, B outside [1, 65535], a row table that is not 16-byte aligned, max_dst_pixels < 1. */
typedef struct {
    uint64_t src, dst;
    int32_t Hs, Ws, Hd, Wd;
} w2l_resize_row;
int w2l_resize_rows_u8(void* stream, int B, const w2l_resize_row* rows, int max_dst_pixels);

/* Row-table JPEG encoding of face crops (preprocess.py:62 `cv2.imwrite(<i>.jpg, fb[j][y1:y2, x1:x2])`: baseline JFIF, 4:2:0,
 * standard Huffman tables, no restart markers).  Row b is a w2l_frame_row: src is the frame u8 [H,W,3] BGR at ANY byte address,
 * the box y1:y2, x1:x2 is the crop, dst is the row's output slot of cap[b] bytes at any byte address.  After the launch
 * dst[0 : lengths[b]] is the complete file of that crop, byte-equal to what libjpeg(-turbo) writes for the same pixels at
 * `quality` (PIL.Image.save(format="JPEG", quality=q, subsampling=2), cv2.imwrite's IMWRITE_JPEG_QUALITY): 623 header bytes (SOI,
 * APP0 JFIF 1.1, DQT luma, DQT chroma, SOF0, DHT DC0 AC0 DC1 AC1, SOS; height at offset 163, width at 165), the entropy stream,
 * EOI.  Rows of different crop sizes share the launch, two rows may name one frame, no pixel outside a box is read.  Two kernel
 * launches per call, whatever B is; the bytes are a function of the pixels alone (integer arithmetic, no run-to-run variation).
 *
 * max_blocks >= the largest 6 * ceil(h / 16) * ceil(w / 16) of the batch (h, w: crop sizes) sizes the launch and the workspace;
 * workspace: device memory, 16-byte aligned, at least w2l_jpeg_workspace_bytes(B, max_blocks) bytes, contents unspecified before
 * and after.  cap, lengths: device int32 [B].
 *
 * A row whose file would not fit cap[b], whose crop has more blocks than max_blocks, or whose crop is higher or wider than 65535
 * gets lengths[b] = -1 and nothing of its slot is written.  Bytes of a slot beyond lengths[b] are unspecified; bytes outside every
 * slot are never written.  No file can exceed 625 + 416 * (its number of blocks) bytes: a block codes at most 22 bits of DC and
 * 63 x 26 bits of AC = 208 bytes, byte stuffing can double that, and header + EOI are 625 (wav2lip_amd/jpeg.py capacity).
 *
 * PRECONDITION: every box is non-empty and inside its frame (0 <= y1 < y2 <= H, 0 <= x1 < x2 <= W), checked by the HOST caller
 * (wav2lip_amd/jpeg.py) as for the other row-table kernels.  Refused with an error code, nothing written: NULL pointers, B outside
 * [1, 65535], a row table that is not 16-byte aligned, quality outside [1, 100], max_blocks outside [1, 2^20], a workspace that
 * is misaligned or too small. */
int w2l_jpeg_encode_rows(void* stream, int B, const w2l_frame_row* rows, const int32_t* cap, int quality, int max_blocks,
                         int32_t* lengths, void* workspace, size_t workspace_bytes);
/* bytes of workspace one w2l_jpeg_encode_rows launch needs; 0 for B outside [1, 65535] or max_blocks outside [1, 2^20] */
size_t w2l_jpeg_workspace_bytes(int B, int max_blocks);
/* host only: the 623 header bytes of an h x w file at `quality` into out[623] (what the kernel copies and patches the size into) */
int w2l_jpeg_header(int h, int w, int quality, uint8_t* out);

/* w2l_jpeg_encode_rows with restart intervals: the frames of a Motion-JPEG stream (inference.py:256-257 `cv2.VideoWriter(...)`,
 * :272 `out.write(f)`: the reference's compressed result video), each frame coded in independent byte-aligned pieces so that a
 * decoder need not walk it serially.  Same arguments, rows and properties as w2l_jpeg_encode_rows; restart_rows >= 1 is libjpeg's
 * restart_in_rows (PIL.Image.save(..., restart_marker_rows=restart_rows)) and the files are byte-equal to libjpeg's:
 *   - 629 header bytes: the 623 of w2l_jpeg_header with DRI (FF DD 00 04 Ri) at offset 609, between the last DHT and SOS;
 *     Ri = min(restart_rows * ceil(w / 16), 65535) MCUs
 *   - at the end of every interval but the last (jchuff.c emit_restart): the last byte filled up with 1 bits, byte stuffing applied
 *     to that byte too (FF becomes FF 00), the marker FF D0+(k mod 8) for interval k, and the three DC predictions back to 0
 *   - dummy blocks keep jccoefct.c's rule inside their MCU; behind the last interval the padding and EOI, no marker.
 * No file can exceed 631 + 416 * blocks + 4 * intervals bytes (intervals = ceil(MCUs / Ri): a padding byte, its stuffed 00 and
 * the marker each; w2l_jpeg_capacity_rst).  workspace: at least w2l_jpeg_workspace_bytes_rst(B, max_blocks) bytes.  Two kernel
 * launches per call, whatever B is.  Refused as w2l_jpeg_encode_rows refuses, and restart_rows < 1. */
int w2l_jpeg_encode_rows_rst(void* stream, int B, const w2l_frame_row* rows, const int32_t* cap, int quality, int max_blocks,
                             int restart_rows, int32_t* lengths, void* workspace, size_t workspace_bytes);
/* 0 for B outside [1, 65535] or max_blocks outside [1, 2^20] */
size_t w2l_jpeg_workspace_bytes_rst(int B, int max_blocks);
/* host only: bytes no file of an h x w image at restart_rows can exceed; 0 for sizes outside [1, 65535] or restart_rows < 1 */
size_t w2l_jpeg_capacity_rst(int h, int w, int restart_rows);
/* host only: the 629 header bytes of an h x w file at `quality` and restart_rows into out[629] */
int w2l_jpeg_header_rst(int h, int w, int quality, int restart_rows, uint8_t* out);

/* Row-table JPEG DECODING of face crops (wav2lip_train.py:66 / color_syncnet_train.py:97 `cv2.imread(fname)` of every <id>.jpg):
 * the read side of w2l_jpeg_encode_rows.  The pixels are byte-equal to what libjpeg(-turbo) decodes with its defaults (PIL's
 * Image.open(...).convert("RGB"), cv2.imread): jpeg_idct_islow, h2v2 "fancy" chroma upsampling (plain 2x2 replication for images of 1 to 4 columns, as
 * libjpeg chooses), ycc_rgb_convert.
 *
 * Accepted class (w2l_jpeg_parse refuses everything else): baseline SOF0, 8-bit samples, three components sampled 2x2, 1x1, 1x1
 * (4:2:0) with Cb and Cr on the same tables, 8-bit quantisers, ONE interleaved scan with Ss = 0, Se = 63, Ah = Al = 0, no restart
 * interval (no DRI, or DRI = 0), JFIF or no APPn segment at all, any valid Huffman tables (not only Annex K's).
 *
 * w2l_jpeg_info: what w2l_jpeg_parse reads from one file's markers (host only, touches no device):
 *   H, W                   image size, each in [1, 65535]
 *   ecs_offset, ecs_bytes  the entropy-coded segment: from behind the SOS header to the EOI marker (eoi = 1), or, where the
 *                          file has no EOI, to its last byte (eoi = 0).  A file cut inside its stream, or ending in a lone
 *                          FF, is then refused by the kernel; one that lacks nothing but the EOI decodes with status 0
 *   quant[2][64]           quantisers of luma and chroma in zigzag order, as the DQT segments carry them
 *   bits[4][16], vals[4][256], nvals[4]   Huffman tables DC luma, AC luma, DC chroma, AC chroma as DHT carries them
 * Return value: 0, or one of the reasons below with w2l_last_error() set; W2L_JPEG_MALFORMED is a file that is no JPEG or is cut
 * inside its header, the others are well-formed files outside the class.  Never reads data[n] or beyond, whatever the
 * segment lengths in the file claim. */
#define W2L_JPEG_MALFORMED (-100)        /* no SOI, a segment running past the file, a missing table or SOF, RSTn without DRI ... */
#define W2L_JPEG_NOT_BASELINE (-101)     /* progressive, extended, lossless or arithmetic-coded (any SOFn but SOF0) */
#define W2L_JPEG_PRECISION (-102)        /* samples that are not 8 bits wide */
#define W2L_JPEG_COMPONENTS (-103)       /* not three components (grayscale, CMYK) */
#define W2L_JPEG_SAMPLING (-104)         /* sampling factors other than 2x2, 1x1, 1x1 (4:4:4, 4:2:2, ...) */
#define W2L_JPEG_RESTART (-105)          /* a restart interval */
#define W2L_JPEG_QUANT16 (-106)          /* 16-bit quantisation tables */
#define W2L_JPEG_SCANS (-107)            /* more than one scan, a scan that is not all three components, or Ss/Se/Ah/Al set */
#define W2L_JPEG_APPN (-108)             /* an APPn segment that is not JFIF / JFXX (Adobe APP14, Exif ...) */
#define W2L_JPEG_SIZE (-109)             /* a height or width of 0 */
#define W2L_JPEG_TABLES (-110)           /* Cb and Cr on different tables, or table ids outside 0..3 */
#define W2L_JPEG_COLORSPACE (-111)       /* no JFIF segment and component ids 'R' 'G' 'B': libjpeg decodes such a file as RGB */
typedef struct {
    int32_t H, W;
    int32_t ecs_offset, ecs_bytes;
    int32_t eoi;
    int32_t nvals[4];
    uint8_t quant[2][64];
    uint8_t bits[4][16];
    uint8_t vals[4][256];
} w2l_jpeg_info;
int w2l_jpeg_parse(const uint8_t* data, size_t n, w2l_jpeg_info* info);

/* host only: the table set of a parsed file in the lookup form the kernel reads (a 9-bit lookahead, then maxcode / valptr of
 * T.81 F.2.2.3 for longer codes; quantisers widened to 16 bits), w2l_jpeg_table_bytes() = 5952 bytes into `out`.  Refused with
 * w2l_last_error() set: (bits, vals) that form no prefix code or oversubscribe the code space (more than 2^l codes of up to l
 * bits), more than 256 symbols, a symbol listed twice, a DC category above 11, a quantiser of 0. */
size_t w2l_jpeg_table_bytes(void);
int w2l_jpeg_build_tables(const w2l_jpeg_info* info, void* out);

/* w2l_jpeg_row, 32 bytes, alignment 16:
 *   bytes  0 ..  7  src (uint64)     device address of the file's entropy-coded segment, at ANY byte address
 *   bytes  8 .. 15  dst (uint64)     device address of the row's output image u8 [H,W,3] BGR, at ANY byte address
 *   bytes 16 .. 19  nbytes (int32)   bytes of the segment (w2l_jpeg_info.ecs_bytes)
 *   bytes 20 .. 27  H, W (int32)     the image's size
 *   bytes 28 .. 31  table (int32)    index of its table set in `tables`
 * tables: n_tables sets of w2l_jpeg_table_bytes() each, back to back, device memory, 16-byte aligned.  Rows of different sizes
 * and table sets share the launch; two rows may name one file.  One memset and three kernel launches per call, whatever B is:
 * entropy decoding (one lane per file; sequential within a file, parallel across files), the inverse DCT, upsampling + colour.
 *
 * After the launch status[b] (device int32 [B]) is 0 and the image complete, or a negative reason and the image's bytes
 * unspecified: -1 bits that are no code of the row's table, -2 a zero run past coefficient 63, -3 a marker other than the stuffed
 * FF 00 (or bytes left over) before the end of the last MCU, -4 the stream ended early, -5 a row the launch cannot take (a size
 * outside [1, 65535], more than max_blocks blocks, nbytes < 1, table outside [0, n_tables)).  Every read of a stream is bounded by
 * its nbytes; a failed row writes nothing outside its own workspace slot and output image and does not affect the other rows.
 *
 * max_blocks >= the largest 6 * ceil(H / 16) * ceil(W / 16) of the batch; workspace: device memory, 16-byte aligned, at least
 * w2l_jpeg_decode_workspace_bytes(B, max_blocks) bytes (192 per block: int16 coefficients and the three sample planes).
 * Refused with an error code, nothing written: NULL pointers, B outside [1, 65535], max_blocks outside [1, 2^20], n_tables
 * outside [1, 65535], rows or tables not 16-byte aligned, a workspace that is misaligned or too small. */
typedef struct {
    uint64_t src, dst;
    int32_t nbytes, H, W, table;
} w2l_jpeg_row;
int w2l_jpeg_decode_rows(void* stream, int B, const w2l_jpeg_row* rows, const void* tables, int n_tables, int max_blocks,
                         int32_t* status, void* workspace, size_t workspace_bytes);
/* 0 for B outside [1, 65535] or max_blocks outside [1, 2^20] */
size_t w2l_jpeg_decode_workspace_bytes(int B, int max_blocks);

/* Decoding of files WITH restart intervals: the frames of a Motion-JPEG video (inference.py:189-215, `cv2.VideoCapture(args.face)`
 * ... `video_stream.read()`, for a compressed --face video) and what w2l_jpeg_encode_rows_rst writes.
 *
 * w2l_jpeg_parse_rst (host only): w2l_jpeg_parse for the same class plus a restart interval: *restart_interval is the DRI value
 * in MCUs (0: none).  ecs_offset / ecs_bytes cover the whole scan, RSTn markers included.
 *
 * w2l_jpeg_restart_segments (host only): the intervals of an entropy-coded segment `ecs` of n_mcus = ceil(H / 16) * ceil(W / 16)
 * MCUs at interval ri.  A data byte FF is always followed by 00, so FF D0..D7 is a marker and one linear pass is exact.  Writes at
 * most `cap` records into `out` (row = 0; offset / nbytes relative to ecs, markers excluded; first_mcu = k * ri) and returns the
 * number of intervals ceil(n_mcus / ri) >= 1, or W2L_JPEG_MALFORMED with w2l_last_error() set: not exactly ceil(n_mcus / ri) - 1
 * markers, marker k not RST(k mod 8), or another marker.  ri = 0: one record covering ecs.  Never reads ecs[ecs_bytes] or beyond.
 *
 * w2l_jpeg_segment, 32 bytes, alignment 16:
 *   bytes  0 ..  3  row (int32)        index of the record's row in `rows`
 *   bytes  4 ..  7  offset (int32)     first byte of the interval, relative to the row's src
 *   bytes  8 .. 11  nbytes (int32)     its bytes (the marker behind it excluded)
 *   bytes 12 .. 15  first_mcu (int32)  the first MCU it codes, in raster order
 *   bytes 16 .. 19  n_mcus (int32)     how many
 *   bytes 20 .. 31  0
 *
 * w2l_jpeg_decode_rows_rst: w2l_jpeg_decode_rows with the entropy pass split over `segments` (device, n_segments records, 16-byte
 * aligned): ONE LANE PER SEGMENT, the lanes of a wave taking consecutive records; a segment starts with its DC predictions at 0
 * and writes the coefficients of its own MCUs only.  A file without restarts is one segment of all its MCUs, so both kinds share
 * a launch.  The inverse DCT and the colour kernel are those of w2l_jpeg_decode_rows.  PRECONDITION (the host caller's, as
 * w2l_jpeg_restart_segments delivers it): the segments of a row do not overlap.
 * status[b]: 0 and the image complete, or the MINIMUM (the most negative) of the reasons of the row's segments (the codes of
 * w2l_jpeg_decode_rows; -5 also for a record whose row, offset, nbytes or MCU range lies outside its row) - a rule that does not
 * depend on the order in which segments finish; a row whose good segments do not add up to its MCUs gets -5.  Every read of a
 * stream is bounded by the segment's bytes inside the row's nbytes; a bad segment leaves other rows intact.
 * Two memsets and four launches per call, whatever B and n_segments are.  workspace: w2l_jpeg_decode_workspace_bytes_rst(B,
 * max_blocks) bytes.  Refused as w2l_jpeg_decode_rows refuses, and n_segments outside [1, 2^24] or a misaligned table. */
typedef struct {
    int32_t row, offset, nbytes, first_mcu, n_mcus;
    int32_t pad[3];
} w2l_jpeg_segment;
int w2l_jpeg_parse_rst(const uint8_t* data, size_t n, w2l_jpeg_info* info, int32_t* restart_interval);
int w2l_jpeg_restart_segments(const uint8_t* ecs, size_t ecs_bytes, int restart_interval, int n_mcus, w2l_jpeg_segment* out, int cap);
int w2l_jpeg_decode_rows_rst(void* stream, int B, const w2l_jpeg_row* rows, const void* tables, int n_tables, int max_blocks,
                             const w2l_jpeg_segment* segments, int n_segments, int32_t* status, void* workspace,
                             size_t workspace_bytes);
size_t w2l_jpeg_decode_workspace_bytes_rst(int B, int max_blocks);

/* ---------------------------------------------------------------- S3FD face detector glue (face_detection/detection/sfd/)
 * The detector's convolutions are w2l_conv_* layers (bias + ReLU, no BatchNorm); these are the ops between them. */

/* bgr u8 [npix][3] -> y fp32 [npix][y_cs]: RGB order (api.py:62 images[..., ::-1]) minus (104,117,123) (detect.py:57),
 * channel 3 zero when y_cs %% 4 == 0 */
int w2l_s3fd_pack(void* stream, long long npix, const uint8_t* bgr, float* y, int y_cs);
/* The row-table form of w2l_s3fd_pack: `frames` is a device table of B addresses (8-byte aligned); entry b is pixel (0,0) of a u8
 * [H,W,3] BGR frame anywhere in device memory, at ANY byte alignment (dword loads where the frame is 4-byte aligned, bytes
 * elsewhere).  Image b of y [B,H,W,y_cs] is what w2l_s3fd_pack writes for that frame, byte for byte: a batch may hold frames of
 * several clips, read where they lie (face_detection/many.py).  B <= 65535, H * W <= 2^29. */
int w2l_s3fd_pack_rows(void* stream, int B, int H, int W, const uint64_t* frames, float* y, int y_cs);
/* The reduced-resolution row-table pack (`--face_det_scale k`: the detector sees cv2.resize(frame, (w // k, h // k)), the resize of
 * inference.py:202-203, while every output frame keeps its size).  Entry b of `frames` is a u8 [Hs,Ws,3] BGR frame at any byte
 * address; image b of y fp32 [B,Hd,Wd,y_cs] is what w2l_s3fd_pack_rows writes for the Hd x Wd frame w2l_resize_rows_u8 makes of
 * it, byte for byte (the equal-size copy, the exact-2x average and the 11-bit bilinear path included) - the reduced frame itself
 * is never stored.  Any (Hd, Wd) is taken, not only (Hs / k, Ws / k).  Refused with an error code, nothing written: a NULL
 * pointer, B outside [1, 65535], a size below 1, Hs * Ws or Hd * Wd above 2^29, a table that is not 8-byte aligned, y not 16-byte
 * aligned, y_cs not a multiple of 4 (a pixel leaves as one 16-byte store; channels >= 4 are left as they are). */
int w2l_s3fd_pack_rows_scaled(void* stream, int B, int Hs, int Ws, int Hd, int Wd, const uint64_t* frames, float* y, int y_cs);
/* F.max_pool2d(x, 2, 2) on NHWC: y [N,H/2,W/2,y_cs] (net_s3fd.py:75-97); C %% 4 == 0 */
int w2l_maxpool2x2(void* stream, int N, int H, int W, int C, const float* x, int x_cs, float* y, int y_cs);
/* L2Norm (net_s3fd.py:6-19): y[row][c] = x[row][c] / (sqrt(sum_c x^2) + 1e-10) * weight[c] */
int w2l_l2norm_scale(void* stream, long long rows, int C, const float* x, int x_cs, const float* weight, float* y, int y_cs);
/* One detection level: cls [B,FH,FW,cls_cs] (ncls = 4: max-out background over the first three, net_s3fd.py:123-126;
 * ncls = 2), reg [B,FH,FW,reg_cs] -> out [B][FH*FW][5] = (x1, y1, x2, y2, softmax score) with the prior of `stride`
 * (detect.py:66-84, bbox.py:91-108, variances 0.1 / 0.2) */
int w2l_s3fd_decode(void* stream, int B, int FH, int FW, int stride, const float* cls, int cls_cs, int ncls, const float* reg,
                    int reg_cs, float* out);
/* Candidate gate + greedy non-maximum suppression per image (sfd_detector.py:39-45: `bboxlist[:, 4] > 0.05`, then bbox.py:44-64
 * `nms(dets, thresh)`): table [B][P][5] = (x1, y1, x2, y2, score) rows (the concatenated w2l_s3fd_decode levels, or any box
 * list); rows with score > gate compete, best score first (equal scores: the later row first - the reference leaves that order
 * to numpy's unstable argsort); a box is dropped when its overlap with a kept one is not <= thresh, the overlap being the
 * reference's float32 expression evaluated operation by operation.  keep [B][P] receives the kept ROW indices of each image in
 * selection order (score descending), counts [B] how many.  scratch: >= 12 * B * P bytes, 8-byte aligned.  P is not bounded;
 * an image with more than 262144 rows ABOVE THE GATE (the alive bitmap of the greedy pass lives in LDS) gets counts = -1 and no
 * keep list: the caller runs that image's suppression elsewhere (wav2lip_amd/face_detection/s3fd.py does, on the host).  Scores
 * of either sign order as floats do. */
int w2l_s3fd_nms(void* stream, int B, int P, const float* table, float gate, float thresh, int* keep, int* counts,
                 void* scratch, long long scratch_bytes);
/* The rect get_detections_for_batch keeps per image (sfd_detector.py:45 + api.py:61-77), from w2l_s3fd_nms's outputs after the
 * caller has resolved any counts = -1 (counts final): the first row of keep[b][:counts[b]] whose score is > thresh, its (x1, y1,
 * x2, y2) clipped at 0 and truncated to int as Python's int() does -> rects [B][4] int32, flags [B] int32: 1 found, 0 no row
 * passes (rect zeros), 2 the host must decide (a coordinate of that row is NaN, +inf or >= 2^31, a kept index lies outside
 * [0, P), or counts[b] is not in [0, P]; rect zeros).  The table is fp32 for either detector precision. */
int w2l_s3fd_first_rect(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh,
                        int* rects, int* flags);
/* w2l_s3fd_first_rect for a detector that ran on a reduced frame: the kept row's x1, x2 are multiplied by sx and its y1, y2 by sy
 * (one fp32 multiply each, round to nearest, no contraction) BEFORE the clip at 0 and the truncation of api.py:61-77, and the
 * "host must decide" flag (NaN, +inf, >= 2^31) is decided on the product.  The caller passes sx = float32(W / Wd) and
 * sy = float32(H / Hd), divided in double and rounded once.  sx = sy = 1 gives w2l_s3fd_first_rect's output byte for byte.
 * Refused: sx or sy that is not finite and positive. */
int w2l_s3fd_first_rect_scaled(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh,
                               float sx, float sy, int* rects, int* flags);

/* Tracked face selection (opt-in `face_track`; the reference takes d[0] of every frame, api.py:61-77 after
 * sfd_detector.py:45, which changes hands between two people in the picture).  Two launches between w2l_s3fd_nms and the box finishes.
 *
 * w2l_s3fd_top_rects: the CANDIDATES of each image - the first K rows of keep[b][:counts[b]], in keep order, whose score is
 * > thresh, each converted as w2l_s3fd_first_rect[_scaled] converts its one row (x * sx, y * sy in fp32, round to nearest, no
 * contraction; sx = sy = 1 gives the unscaled bits; clip at 0; truncation) -> cands [B][K][4] int32 (x1, y1, x2, y2), unused
 * slots zeros, ncand [B], flags [B]: 1 with at least one candidate, 0 with none, 2 the host must decide (no candidates written) -
 * counts[b] not in [0, P], a keep entry outside [0, P) among those examined (up to and including the K-th passing row; rows after
 * it are not looked at), or a coordinate of a taken candidate that is NaN or, after the clip and the truncation, above 32767 (so
 * +inf and >= 2^31 too).  That bound keeps every product of the track exact in int64.  Zero-area candidates are kept.  Candidate 0
 * of an image flagged 1 is w2l_s3fd_first_rect's rect.  Refused: a NULL pointer, B or P < 1, B * P * 5 >= 2^31, sx or sy not
 * finite and positive, K outside 1..16.
 *
 * w2l_face_track_segments: one candidate per frame, followed through the frames of a segment in order.  cands [n_rows][K][4],
 * ncand [n_rows] and cflags [n_rows] are arenas w2l_s3fd_top_rects filled (coordinates in 0..32767); rects [n_rows][4] and
 * flags [n_rows] come out in w2l_s3fd_first_rect's format, so the four box finishes below take them unchanged.
 *
 * w2l_track_segment, 16 bytes, the table 16-byte aligned:
 *   bytes 0..7   int32 row0, n     the segment's rows [row0, row0 + n) of the arenas (n = 0: no frame; the state is carried on)
 *   bytes 8..15  int32 slot, seen  slot -1: no carried state (a clip).  slot >= 0: the state is read from state[slot] when
 *                                  seen > 0 (frames of this stream before the segment; 0: a fresh state) and ALWAYS written back
 *
 * The state is (ref rect, has, missed), fresh = no track.  state [n_slots][8] int32 = (x1, y1, x2, y2, has, missed, 0, 0), zeros
 * without a track.  With pick 0 score, 1 largest, 2 left, 3 right; L in 0..250 missed frames tolerated; q in 1..256 (min IoU q/256):
 *   - a frame flagged neither 0 nor 1: flag 2, rect zeros, the state unchanged.
 *   - inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)), union = area(c) + area(ref) - inter, area = (x2 - x1) *
 *     (y2 - y1), no + 1, all integers (not the float expression of the NMS).  Candidate c OVERLAPS when inter > 0 and
 *     inter * 256 >= q * union.
 *   - with a track: the overlapping candidate of the largest IoU (inter_a * union_b > inter_b * union_a in int64; ties to the
 *     lower index) is the frame's rect, flag 1, becomes ref, missed = 0.  None: missed += 1; while missed <= L the frame is flag 0
 *     with zeros; once missed > L the track is dropped and the SAME frame seeds a new one.
 *   - without a track: no candidate -> flag 0, zeros; else the seed by pick - candidate 0; the largest area; the smallest
 *     x1 + x2; the largest x1 + x2; every tie to the lower index - is the rect, flag 1, ref, has = 1, missed = 0.
 * With L = 0 a frame that has a candidate is never flag 0.  status [n_seg] int32: 0, or 3 for a segment with rows outside
 * [0, n_rows), n < 0, seen < 0 or a slot outside [-1, n_slots) - nothing else of it is read or written.  A segment writes its own
 * rows and its own slot's eight words only.  Refused: a NULL pointer (state may be NULL with n_slots = 0), n_seg < 1, n_rows < 0,
 * K outside 1..16, pick, L or q outside their ranges, a segment table, cands or rects that is not 16-byte aligned. */
typedef struct {
    int32_t row0, n, slot, seen;
} w2l_track_segment;
int w2l_s3fd_top_rects(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh, float sx,
                       float sy, int K, int32_t* cands, int32_t* ncand, int32_t* flags);
int w2l_face_track_segments(void* stream, int n_seg, const w2l_track_segment* segs, const int32_t* cands, const int32_t* ncand,
                            const int32_t* cflags, int n_rows, int K, int pick, int L, int q, int32_t* state, int n_slots,
                            int32_t* rects, int32_t* flags, int32_t* status);

/* The per-clip finish of face_detect (inference.py:90-104 pads + clipping + "Face not detected", :59-66 get_smoothened_boxes;
 * evaluation/gen_videos_from_filelist.py:35-42, :61-77 is the same code) for many clips in one launch.  rects [R][4] = (x1, y1, x2, y2)
 * and flags [R] are arenas w2l_s3fd_first_rect filled (its two output pointers aimed at the rows of each batch); segment k is
 * one clip: rows [row0, row0 + n) of them, frames of H x W.
 *
 * w2l_box_segment, 16 bytes, the table 16-byte aligned:
 *   bytes 0..7   int32 row0, n   the clip's rows of the arenas (n <= 0: nothing is read or written, status (0, 0))
 *   bytes 8..15  int32 H, W      its frame size
 *
 * boxes [R][4] = (y1, y2, x1, x2), the `coords` order face_detect returns: (max(0, y1 - top), min(H, y2 + bottom),
 * max(0, x1 - left), min(W, x2 + right)) - a negative pad or a rect beyond the frame is not pulled back from the other side, as
 * there - then for T >= 1 get_smoothened_boxes exactly: in place and in row order, window [i, i + T) while i + T <= n, else
 * Python's boxes[n - T:] (for n < T the negative start wraps and is clipped at 0), every mean an integer sum divided in fp64 and
 * truncated towards zero on assignment.  T = 0: no smoothing.  0 <= T <= 64.
 * status [n_seg][2] = (code, row inside the segment): 2 when a row is flagged 2 (the host must decide; the first such row - the
 * detector meets it before face_detect looks for None), else 1 when a row is flagged 0 (no face; the first such row), else
 * (0, 0).  For a non-zero code the segment's boxes are zeros.  A segment reads and writes its own rows only. */
typedef struct {
    int32_t row0, n, H, W;
} w2l_box_segment;
int w2l_face_boxes_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags,
                            int top, int bottom, int left, int right, int T, int32_t* boxes, int32_t* status);

/* The same finish (inference.py:59-66, :90-104) for many LIVE streams, one launch per tick: frames arrive a few at a time and a
 * box leaves as soon as it is final.  get_smoothened_boxes looks forward - box i <= n - T is the mean of the unsmoothed rows
 * i .. i + T - 1 - so it is final once T - 1 more frames are there; only the last T - 1 boxes of a video depend on its end.  A
 * stream carries its last max(T, 1) RAW rects (x1, y1, x2, y2) from tick to tick in a slot of carry [n_slots][64][4] int32.
 *
 * w2l_box_stream_segment, 32 bytes, the table 16-byte aligned: one stream that takes part in the tick
 *   bytes 0..7    int32 row0, n_new   its new rows [row0, row0 + n_new) of the rect / flag arenas (n_new = 0: an empty tick)
 *   bytes 8..15   int32 H, W          its frame size
 *   bytes 16..23  int32 slot, seen    its carry slot; frames of this stream finished before this tick
 *   bytes 24..31  int32 closed, out0  1: the video ended with this tick; first row of the segment in boxes
 *
 * With n = seen + n_new the rows held are [the slot's first min(seen, max(T, 1)) rows][the new rows].  While open the segment
 * writes the boxes of frames [max(0, seen - T + 1), max(0, n - T + 1)) by the forward rule (T = 0: the new frames unsmoothed;
 * T = 1: each frame's own truncated mean).  With closed it writes every remaining frame - [max(0, seen - T + 1), n) - by
 * w2l_face_boxes_segments' rule on the WHOLE length n: the forward rule below n - T, then in order over the window
 * boxes[n - T:] (n < T: from max(0, 2n - T)), whose entry n - T is computed again from raw rows.  So the boxes of a stream,
 * tick after tick, are w2l_face_boxes_segments' of the finished video however it was cut.  Then the last min(n, max(T, 1)) raw
 * rects go back into the slot.  boxes rows [out0, out0 + count) = (y1, y2, x1, x2), count as above.
 * status [n_seg][2] = (code, absolute frame index): 2 when a NEW row is flagged neither found nor none (the first such row; it
 * wins over an earlier "none"), else 1 when a new row is flagged 0 (no face; the first), else (0, 0).  For a non-zero code no
 * box of the segment is written and its slot is left as it was.  A segment touches its own arena rows, output rows and slot only.
 * segs_host is the same table in host memory (the staging copy): it is checked before anything is launched - n_new, seen not
 * negative, seen + n_new < 2^31, slot in [0, n_slots) and named once, rows inside n_rows, output rows inside n_out and disjoint -
 * and refused with w2l_last_error set.  The kernel reads segs (device) and does not follow a segment that fails those bounds:
 * status (3, 0), nothing else written.  Also refused: a NULL pointer, n_seg < 1, T outside 0..64, a misaligned table. */
typedef struct {
    int32_t row0, n_new, H, W, slot, seen, closed, out0;
} w2l_box_stream_segment;
int w2l_face_boxes_stream(void* stream, int n_seg, const w2l_box_stream_segment* segs_host, const w2l_box_stream_segment* segs,
                          const int32_t* rects, const int32_t* flags, int n_rows, int32_t* carry, int n_slots, int top, int bottom,
                          int left, int right, int T, int32_t* boxes, int n_out, int32_t* status);

/* The two finishes above with the opt-in pass-through for frames without a face (`no_face_hold`; not the
 * reference's behaviour).  A row flagged 0 no longer decides its clip.  With hold in 0..250:
 *   - a detected frame is BOXED with its own rect; an undetected frame i is boxed with the raw rect of the last detected frame
 *     p < i while i - p <= hold; any other frame (every frame before the first detection too) is a GAP.  The hold looks back only.
 *   - maximal sequences of boxed frames are runs, and each run is finished exactly as w2l_face_boxes_segments finishes a clip
 *     that consists of the run's frames alone: pads, clipping, then get_smoothened_boxes over the run.
 * valid [R] is 1 for a boxed row and 0 for a gap row, whose box is zeros.  A clip with no undetected frame is one run: its boxes
 * are w2l_face_boxes_segments' bytes.
 *
 * w2l_face_boxes_runs takes w2l_face_boxes_segments' table and arenas of n_rows rows.  status [n_seg][2]: (2, row) when a row
 * is flagged neither found nor none (boxes and valid of the segment zeros), (3, 0) for a segment with rows outside
 * [0, n_rows) - nothing of it is read or written - else (0, 0); code 1 does not occur.  Refused: a NULL pointer, n_seg < 1,
 * n_rows < 0, T outside 0..64, hold outside 0..250, a misaligned table.
 *
 * w2l_face_boxes_stream_runs is the per-tick form, with w2l_face_boxes_stream's table, checks, status (code 1 does not occur) and
 * range: the frames a tick writes are the same [max(0, seen - T + 1), closed ? n : max(0, n - T + 1)) (T = 0 as T = 1), so a gap
 * frame leaves in the tick in which a boxed one would.  A boxed frame of the range takes the forward mean when its next T - 1
 * frames are boxed, else the tail rule of its run, whose end b is then known (frame b is a gap, or the video is closed).  A run may
 * have ended up to T - 2 frames before the tick's first new frame and its tail reads raw rows back to b - T, so the carry holds
 * the last 2 * max(T, 1) frames: carry [n_slots][644] int32, a slot being 128 rows of (x1, y1, x2, y2, boxed) - the held-filled
 * raw rect, zeros for a gap - of which the first min(seen, 2 * max(T, 1)) are in use, oldest first, then 4 words: the number
 * of frames since the last detected one (0 when the last frame was detected; 251 for anything above 250 and before the first
 * detection), and three zeros.  The boxes and valid of a stream, tick after tick, are w2l_face_boxes_runs' of the finished video
 * however it was cut.  valid rows [out0, out0 + count) lie beside the box rows. */
int w2l_face_boxes_runs(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags, int n_rows,
                        int top, int bottom, int left, int right, int T, int hold, int32_t* boxes, int32_t* valid, int32_t* status);
int w2l_face_boxes_stream_runs(void* stream, int n_seg, const w2l_box_stream_segment* segs_host, const w2l_box_stream_segment* segs,
                               const int32_t* rects, const int32_t* flags, int n_rows, int32_t* carry, int n_slots, int top, int bottom,
                               int left, int right, int T, int hold, int32_t* boxes, int32_t* valid, int n_out, int32_t* status);

/* The span rule for FINISHED clips (opt-in `track_spans`; what the real-video scorer needs, not the reference's
 * code: evaluation/scores_LSE/calculate_scores_real_videos.py leaves it to syncnet_python's run_pipeline.py): the stretches of a
 * segment in which the followed face is present.  Where the hold above looks back, this rule looks forward to the next detection,
 * so a live stream cannot use it.  Over w2l_face_boxes_segments' table (with `scene_cuts` a segment is a shot; its H and W are
 * not read) and the arenas rects [n_rows][4] = (x1, y1, x2, y2), flags [n_rows] that w2l_s3fd_first_rect or
 * w2l_face_track_segments fill, integers only, per segment of n rows:
 *   - a row flagged 1 is DETECTED.  For detected rows p < q with no detected row between them and 2 <= q - p <= bridge + 1 every
 *     row p < i < q is BRIDGED: each coordinate is floor((r_p * (q - i) + r_q * (i - p)) / (q - p)) in int64.  Every other row -
 *     before the first detection, after the last one, inside a longer miss - is a gap.
 *   - a SPAN is a maximal sequence of detected and bridged rows; it begins and ends on a detected row.  With L its length and
 *     sw = sum(x2 - x1), sh = sum(y2 - y1) over its rects (int64) it is KEPT iff L >= min_len and max(sw, sh) >= min_size * L.
 *   - rects_out / flags_out (the format of the inputs): the rows of kept spans have flag 1 and the detected or bridged rect, every
 *     other row flag 0 and zeros.  w2l_face_boxes_runs with hold 0 finishes them as they are: pads, clipping, smoothing per span.
 *   - spans [n_rows][4]: the t-th kept span of segment k, in order, is row row0 + t = (its first row counted from the segment's
 *     first, L, its number of detected rows, 0); the segment's span rows from the kept count on are zeros.
 * status [n_seg][2]: (0, number of kept spans); (2, row) when a row is flagged neither 0 nor 1 - the first such row; rects_out and
 * flags_out of the segment are then copies of the input, so that the finish reports the same row, and its span rows are not
 * written; (3, 0) for a segment with rows outside [0, n_rows) - nothing of it is read or written.  n <= 0: (0, 0), nothing else
 * touched.  A segment writes its own rows of the three output arenas and its own status only; the outputs must not overlap the
 * inputs.  Refused: a NULL pointer, n_seg < 1, n_rows < 0, bridge outside 0..250, min_len outside 1..2^30, min_size outside
 * 0..32767, a table, rects, rects_out or spans that is not 16-byte aligned. */
int w2l_face_spans_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags, int n_rows,
                            int bridge, int min_len, int min_size, int32_t* rects_out, int32_t* flags_out, int32_t* spans,
                            int32_t* status);

/* Every face of a segment (opt-in `all_faces`; what syncnet_python's run_pipeline.py does before
 * evaluation/scores_LSE/calculate_scores_real_videos.py:38-40 prints a line per face track): w2l_face_track_segments' rule with F
 * track slots at once.  Over w2l_face_boxes_segments' table (with `scene_cuts` a segment is a shot; H and W are not read) and the
 * arenas cands [n_rows][K][4], ncand [n_rows], cflags [n_rows] that w2l_s3fd_top_rects fills (coordinates in 0..32767, so every
 * product is exact in int64), integers only, per segment of n rows.  F in 1..16 slots, K in 1..16, L in 0..250 missed frames
 * tolerated, q in 1..256 (min IoU q/256).  inter, union and OVERLAPS are w2l_face_track_segments': no + 1, inter > 0 and
 * inter * 256 >= q * union.  The state is F slots of (ref rect, alive, missed), all free at the segment's start; frames in order:
 *   1. a frame flagged neither 0 nor 1: all F rows of the frame get flag 2 and zeros; the state is left alone, missed not counted.
 *   2. m = ncand clipped to [0, K] for a frame flagged 1, else 0.
 *   3. matching, best pair first: among the pairs (alive slot s, candidate c < m) that overlap, the pair of the largest IoU
 *      (inter_a * union_b > inter_b * union_a in int64; ties to the lower slot, then to the lower candidate) is matched - the
 *      slot's ref becomes the candidate, missed = 0 - and slot and candidate leave the contest; again until no overlapping pair
 *      is left.  (Not slot order: two faces whose boxes cross get the nearer box each.)
 *   4. misses: every alive slot that was not matched does missed += 1 and is freed once missed > L.
 *   5. seeds: the unclaimed candidates, in index order, each take the lowest free slot - one freed in step 4 of this frame
 *      counts as free: ref = candidate, alive, missed = 0, started += 1.  Without a free slot the candidate is dropped, dropped += 1.
 *   6. slot t's row of the frame: flag 1 and the slot's rect if it was matched or seeded in this frame, else flag 0 and zeros.
 * rects_out [F][n_rows][4] and flags_out [F][n_rows]: slot t's arena is the t-th block of n_rows rows, in w2l_s3fd_first_rect's
 * format, so w2l_face_spans_segments and the box finishes take a table of F * n_seg segments (row0 + t * n_rows) over them as
 * they are.  With F = 1 slot 0 is w2l_face_track_segments with pick 0 and the same K, L, q, byte for byte.  Two tracks that use
 * one slot one after the other are at least L rows of flag 0 apart - exactly L when the slot is seeded again in the frame that
 * freed it, L + 1 or more otherwise - so a span rule with bridge < L never joins them, and one with bridge = L joins exactly the
 * tracks of a slot that was freed and seeded in one frame.
 * status [n_seg][4] = (code, started, dropped, the largest number of slots alive after a frame): code 0, or 3 for a segment
 * whose rows leave [0, n_rows) or with n < 0 - (3, 0, 0, 0), nothing else of it is read or written.  n = 0: (0, 0, 0, 0).  A
 * segment writes its own rows of the F arenas and its own status only; no atomics, bit-reproducible.  Refused: a NULL pointer,
 * n_seg < 1, n_rows < 0, K, F, L or q outside their ranges, F * n_rows >= 2^29, a table, cands or rects_out that is not 16-byte
 * aligned. */
int w2l_face_tracks_all_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* cands, const int32_t* ncand,
                                 const int32_t* cflags, int n_rows, int K, int F, int L, int q, int32_t* rects_out, int32_t* flags_out,
                                 int32_t* status);

/* Key-frame detection (opt-in `det_stride`; not the reference's behaviour, which looks at every frame): the
 * detector saw only the KEY frames of a segment and this launch writes the rects and flags of all its frames, in
 * w2l_s3fd_first_rect's format, so that the track, the span rule and the four box finishes above run as they are.  With a stride
 * N in 1..32 a segment of n >= 1 frames (a clip; with `scene_cuts` a shot) has the key frames 0, N, 2N, ... below n, and n - 1:
 * m = (n - 1 + N - 1) / N + 1 of them, key j at frame pos(j) = min(j * N, n - 1).  key_rects [n_key_rows][4] = (x1, y1, x2, y2)
 * and key_flags [n_key_rows] are COMPACT arenas, one row per key frame, that w2l_s3fd_first_rect or w2l_face_track_segments
 * filled; rects [n_rows][4] and flags [n_rows] are the full arenas.  Integers only.
 *
 * w2l_stride_segment, 16 bytes, the table 16-byte aligned:
 *   bytes 0..3    int32 key_row0   the segment's key rows [key_row0, key_row0 + m) of the key arenas
 *   bytes 4..11   int32 row0, n    its rows [row0, row0 + n) of the full arenas (n <= 0: nothing is read or written, status 0)
 *   bytes 12..15  int32 zero       not read
 *
 *   - frame pos(j) takes key row j's rect and flag as they are (0 none, 1 found, 2 the host must decide).
 *   - a frame i with p = pos(j) < i < q = pos(j + 1): if both keys are flagged 1, flag 1 and every coordinate
 *     floor((r_p * (q - i) + r_q * (i - p)) / (q - p)) in int64 - w2l_face_spans_segments' formula; else flag 0 and zeros.  A flag
 *     2 stays on its key row alone, where the finish meets it.
 * So a missed key leaves 2N - 1 rows of flag 0 (fewer at the segment's end).  With N = 1 every frame is a key and the launch is a
 * copy; callers do not launch it then.  status [n_seg] int32: 0, or 3 for a segment whose key rows leave [0, n_key_rows) or whose
 * rows leave [0, n_rows) - nothing else of it is read or written.  One thread per row, rows found by a division: a segment may be
 * longer than a workgroup.  A segment writes its own rows (each rect one 16-byte store) and its own status only; the outputs must
 * not overlap the inputs; no atomics, bit-reproducible.  Refused: a NULL pointer, n_seg < 1, N outside 1..32, n_key_rows < 0,
 * n_rows < 0, a table, key_rects or rects that is not 16-byte aligned. */
typedef struct {
    int32_t key_row0, row0, n, zero;
} w2l_stride_segment;
int w2l_face_rects_expand_segments(void* stream, int n_seg, const w2l_stride_segment* segs, int N, const int32_t* key_rects,
                                   const int32_t* key_flags, int n_key_rows, int32_t* rects, int32_t* flags, int n_rows,
                                   int32_t* status);

/* Scene-cut detection (opt-in `scene_cuts`; not the reference's behaviour, which treats a clip as one take): where
 * the shots of a clip are, decided on the device from the frames the detector reads.  A shot then is a segment of the track and of
 * the box finishes above, which stay as they are.  With one threshold in [1/256, 1), quantised as q = int(thresh * 256) in 1..255:
 *   1. signature: a frame is H * W * 3 contiguous bytes, BGR interleaved; byte j belongs to channel j % 3 and bin byte >> 3;
 *      sig[c * 32 + b] is a uint32 count - 96 words per frame, every channel sums to H * W.  Integers only, no luma, no float.
 *   2. distance: D(i) = sum_k |sig_i[k] - sig_{i-1}[k]|, in 0 .. 6 * H * W.
 *   3. cut: frame i >= 1 of a clip starts a new shot iff D(i) * 256 > q * 6 * H * W in int64; frame 0 never does.  The rule looks
 *      one frame back only (causal).  Gradual transitions - fades, dissolves - are not detected.
 *
 * w2l_frame_hist_rows: `frames` is the address table w2l_s3fd_pack_rows takes (8-byte aligned; entry b = pixel (0,0) of a u8
 * [H,W,3] frame at ANY byte address; an address may repeat) -> sig [B][96] uint32 (4-byte aligned; callers offset the pointer into
 * an arena).  The rows are zeroed on the stream and then added to with integer atomics: the words are independent of the launch
 * geometry and bit-reproducible.  No byte outside [frames[b], frames[b] + H * W * 3) is loaded.  Refused: a NULL pointer, B < 1, H or
 * W < 1, 6 * H * W >= 2^31, a misaligned table or sig.
 *
 * w2l_scene_cuts: over w2l_face_boxes_segments' table, segment k = one clip, rows [row0, row0 + n) of sig [n_rows][96] with
 * frames of H x W.  cuts [n_rows] int32: 1 where the row starts a new shot, a segment's first row always 0; dist [n_rows] int32 = D,
 * 0 on a segment's first row (dist may be NULL).  status [n_seg] int32: 0, or 3 for a segment whose rows leave [0, n_rows) or whose
 * H, W are below 1 or 6 * H * W >= 2^31 - nothing of such a segment is read or written.  n <= 0: status 0, nothing else touched.
 * Refused: a NULL pointer other than dist, n_seg < 1, n_rows < 0, q outside 1..255, a table that is not 16-byte aligned. */
int w2l_frame_hist_rows(void* stream, int B, int H, int W, const uint64_t* frames, uint32_t* sig);
int w2l_scene_cuts(void* stream, int n_seg, const w2l_box_segment* segs, const uint32_t* sig, int n_rows, int q, int32_t* cuts,
                   int32_t* dist, int32_t* status);

/* The opt-in bf16-storage detector (face_detection/s3fd.py, precision="bf16"): the backbone convolutions are w2l_convb layers
 * (scale 1, shift = bias, ReLU); these are the ops between them and the fused detection head.  Tensors are NHWC bf16 with channel
 * strides that are multiples of 8, 16-byte aligned; no buffer may reach 2 GiB (the convb rule: split the batch). */
/* bgr u8 [npix][3] -> y bf16 [npix][y_cs]: the values of w2l_s3fd_pack (api.py:62 + detect.py:57, integers with |v| <= 152, so
 * exact), channels 3 .. y_cs-1 zero */
int w2l_s3fd_pack_bf16(void* stream, long long npix, const uint8_t* bgr, void* y, int y_cs);
/* The row-table form (w2l_s3fd_pack_rows): image b of y bf16 [B,H,W,y_cs] is what w2l_s3fd_pack_bf16 writes for the frame at
 * frames[b], byte for byte */
int w2l_s3fd_pack_rows_bf16(void* stream, int B, int H, int W, const uint64_t* frames, void* y, int y_cs);
/* w2l_s3fd_pack_rows_scaled for the bf16 detector: y bf16 [B,Hd,Wd,y_cs], y_cs %% 8 == 0, channels 3 .. y_cs-1 zero; the values
 * are integers with |v| <= 152, exact in bf16.  Byte-equal to w2l_resize_rows_u8 followed by w2l_s3fd_pack_rows_bf16. */
int w2l_s3fd_pack_rows_scaled_bf16(void* stream, int B, int Hs, int Ws, int Hd, int Wd, const uint64_t* frames, void* y, int y_cs);
/* F.max_pool2d(x, 2, 2) on bf16 NHWC (net_s3fd.py:75-97, floor semantics): bit-equal to torch on the same tensor; C %% 8 == 0 */
int w2l_maxpool2x2_bf16(void* stream, int N, int H, int W, int C, const void* x, int x_cs, void* y, int y_cs);
/* L2Norm (net_s3fd.py:6-19) on bf16 rows: sum of squares and x / (sqrt(.) + 1e-10) * weight[c] in fp32 (weight fp32 [C]),
 * one RNE rounding on the store; C %% 8 == 0 */
int w2l_l2norm_scale_bf16(void* stream, long long rows, int C, const void* x, int x_cs, const float* weight, void* y, int y_cs);
/* One detection level fused (net_s3fd.py:99-126 + detect.py:66-84): the conf (ncls = 4 or 2) and loc (4) 3x3 convolutions of
 * bf16 features x [B,FH,FW,x_cs] as ONE contraction (bf16 MFMA, fp32 accumulation, + fp32 bias), decoded from the accumulators
 * with w2l_s3fd_decode's operations into table fp32 [B][FH*FW][5] = (x1, y1, x2, y2, score).  The handle owns the weights rounded
 * to bf16 once: conf_w [ncls][cin][3][3], loc_w [4][cin][3][3] fp32 device tensors, biases fp32 [ncls] / [4] or NULL (zero);
 * cin %% 32 == 0.  update re-packs them (asynchronous on `stream`). */
typedef struct w2l_s3fd_headb w2l_s3fd_headb_t;
int w2l_s3fd_headb_create(int cin, int ncls, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                          void* stream, w2l_s3fd_headb_t** out);
int w2l_s3fd_headb_update(w2l_s3fd_headb_t* h, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                          void* stream);
int w2l_s3fd_headb_destroy(w2l_s3fd_headb_t* h);
int w2l_s3fd_headb_decode(const w2l_s3fd_headb_t* h, void* stream, int B, int FH, int FW, int stride, const void* x, int x_cs,
                          float* table);

/* ---------------------------------------------------------------- audio */

/* A mel context owns the device copies of the constant tables: the Slaney mel basis fp32 [80][401] and the
 * periodic Hann window f64 [800] (both built once by the host, wav2lip_amd/audio.py, exactly as
 * librosa.filters.mel / scipy.signal.get_window build them) plus the DFT twiddles.
 * hparams fixed to hparams.py:32-69 (n_fft 800, hop 200, win 800, sr 16000, 80 mels, fmin 55, fmax 7600,
 * preemphasis 0.97, ref 20 dB, min -100 dB, symmetric, max_abs 4). */
typedef struct w2l_mel w2l_mel_t;
int w2l_mel_create(const float* mel_basis_host, const double* window_host, w2l_mel_t** out);
int w2l_mel_destroy(w2l_mel_t* m);
int w2l_mel_num_frames(long long nsamples);            /* 1 + nsamples/200 */
/* wav fp32 [nsamples] (device) -> mel fp32 [80][T] row-major (as audio.melspectrogram returns it) */
int w2l_melspectrogram(const w2l_mel_t* m, void* stream, const float* wav, long long nsamples, float* mel);
/* The same spectrogram, incrementally and for MANY streams in one launch (wav2lip_amd/streaming.py): one workgroup per entry of
 * the column table computes column `col` of stream `stream` from the samples the stream still holds, with the arithmetic of
 * w2l_melspectrogram (one shared device function), so that a column equals the same column of the whole signal bit for bit once
 * it is final: on an open stream (total = -1) when col*200 + 400 <= the samples fed so far (column 0: 401 samples), on a closed
 * one (total = its length, > 400) every column 0 .. total/200.  Sample index j of a column: j < 0 reads -j; on a closed stream
 * j >= total reads 2*(total-1) - j.  The caller checks that [first, first + held) covers what the listed columns read; the
 * kernel clamps every index into that range and skips entries whose stream index, sample count or window position is out of
 * range, so a wrong table gives wrong numbers, never a fault.  Tables live in device memory, 16-byte aligned.
 *
 * w2l_mel_stream, 48 bytes, alignment 16:
 *   offset  0  uint64 samples  device address of the held samples, fp32 [held]
 *   offset  8  int64  first    absolute index (in the stream's signal) of samples[0]
 *   offset 16  int64  total    the signal's length once the stream is closed, -1 while it is open
 *   offset 24  uint64 window   device address of the destination spectrogram window, fp32 [80][cap]
 *   offset 32  int32  held     number of samples held
 *   offset 36  int32  cap      columns of the window
 *   offset 40  int64  col0     absolute column that sits at index 0 of the window
 * w2l_mel_col, 16 bytes, alignment 16:
 *   offset  0  int32  stream   row of the stream table
 *   offset  4  int32  rsv      unused
 *   offset  8  int64  col      absolute column; written to window[m][col - col0], m = 0..79 */
typedef struct {
    uint64_t samples;
    int64_t first, total;
    uint64_t window;
    int32_t held, cap;
    int64_t col0;
} w2l_mel_stream;
typedef struct {
    int32_t stream, rsv;
    int64_t col;
} w2l_mel_col;
/* 1 <= nstreams <= 65535, 1 <= ncols <= 1048576; non-zero with w2l_last_error() set otherwise, or for a NULL / misaligned table */
int w2l_mel_stream_cols(const w2l_mel_t* m, void* stream, const w2l_mel_stream* streams, int nstreams, const w2l_mel_col* cols,
                        int ncols);
/* mel [80][T] + starts int32[B] (device) -> out fp32 [B][80][16][out_cs] channel 0 (others zero up to c_zero_to) */
int w2l_mel_gather(void* stream, const float* mel, int T, const int32_t* starts, int B, float* out,
                   int out_cs, int c_zero_to);
/* the same windows as bf16 (each value rounded once, RNE) for the bf16-storage generator: out bf16 [B][80][16][out_cs] */
int w2l_mel_gather_bf16(void* stream, const float* mel, int T, const int32_t* starts, int B, void* out,
                        int out_cs, int c_zero_to);

/* w2l_mel_gather / w2l_mel_gather_bf16 with one spectrogram per row (w2l_mel_row above): the mel chunking of
 * evaluation/gen_videos_from_filelist.py:176-183 for rows of several clips in one batch */
int w2l_mel_gather_rows(void* stream, const w2l_mel_row* rows, int B, float* out, int out_cs, int c_zero_to);
int w2l_mel_gather_rows_bf16(void* stream, const w2l_mel_row* rows, int B, void* out, int out_cs, int c_zero_to);

/* Sample-rate conversion of audio.load_wav (audio.py:9-10 -> librosa.core.load(path, sr=16000) -> resampy.resample(...,
 * filter='kaiser_best')).  x fp32 [n_in], tr f64 [n_out] = the interpolator's time register at every output sample (the host
 * accumulates 1/sample_ratio by repeated float64 addition, as the reference loop does), win / delta f64 [nwin] = the filter's
 * half window (pre-scaled by sample_ratio when < 1) and its first differences, num_table = table samples per zero crossing;
 * y fp32 [n_out].  All pointers are device memory.  Bit-exact with the loop order and the per-term float32 rounding of
 * resampy's resample_f. */
int w2l_resample_sinc(void* stream, const float* x, int n_in, const double* tr, int n_out, double sample_ratio,
                      const double* win, const double* delta, int nwin, int num_table, float* y);

/* The same conversion, incrementally and for MANY streams in one launch (wav2lip_amd/streaming.py): the streams may have
 * different source rates, each with its own filter tables.  With K = nwin / index_step an output sample t whose time register
 * has the integer part n reads the source samples n - K + 1 .. n + K, so on an open stream (src_total = -1) that holds m samples
 * it is FINAL - bit-equal to output t of the whole signal - once n + K <= m - 1; on a closed stream (src_total = its length N,
 * n_res = int(N * ratio)) the wings are cut by the end as w2l_resample_sinc cuts them, and the outputs t >= n_res are written as
 * 0 (librosa's fix_length pads at most one).  One workgroup per block entry, one thread per output: thread j starts from the
 * block's time register tr0 (the host's, by repeated float64 addition) and adds `inc` j times, the reference loop's additions in
 * its order.  A block with copy != 0 copies its outputs from the stream's `carry` buffer (the tail of its previous destination)
 * instead of computing them.  The caller lists final outputs only and checks that [src_first, src_first + src_held) covers what
 * they read; the kernel clamps nothing: an output whose reads leave the held samples, whose stream index is out of range or
 * whose place is outside the destination is skipped, so a wrong table writes nothing, never a fault.  Tables live in device
 * memory, 16-byte aligned; `streams_host` is the host's copy of the stream table (the staging buffer), which the entry point
 * checks before it launches.
 *
 * w2l_resample_stream_entry, 128 bytes, alignment 16:
 *   at   0  uint64  src         device address of the held source samples, fp32 [src_held]
 *   at   8  int64   src_first   absolute index (in the stream's source signal) of src[0]
 *   at  16  int64   src_total   the source signal's length once the stream is closed, -1 while it is open
 *   at  24  int64   n_res       int(src_total * ratio) once the stream is closed, -1 while it is open
 *   at  32  uint64  dst16       device address of the destination, fp32 [dst_cap]
 *   at  40  int64   dst_first   absolute index (in the resampled signal) of dst16[0]
 *   at  48  uint64  win         device address of the half window, f64 [nwin] (scaled by the ratio when it is < 1)
 *   at  56  uint64  delta       device address of its first differences, f64 [nwin], last entry 0
 *   at  64  uint64  carry       device address of the previous destination's samples, fp32 [carry_held], or 0
 *   at  72  int64   carry_first absolute index of carry[0]
 *   at  80  float64 scale       min(1, ratio)
 *   at  88  float64 inc         1 / ratio, the time register's increment
 *   at  96  int32   src_held    source samples held
 *   at 100  int32   dst_cap     samples of the destination
 *   at 104  int32   index_step  int(scale * num_table), >= 1
 *   at 108  int32   nwin        entries of win and delta
 *   at 112  int32   carry_held  samples behind `carry`
 *   at 116  int32   unused      [3]
 * w2l_resample_block, 32 bytes, alignment 16:
 *   at   0  int32   stream      row of the stream table
 *   at   4  int32   count       outputs of this block, 1 .. 128
 *   at   8  int64   t0          absolute index of its first output; output t0 + j goes to dst16[t0 + j - dst_first]
 *   at  16  float64 tr0         time register of output t0
 *   at  24  int32   copy        non-zero: copy the outputs from `carry` instead of computing them
 *   at  28  int32   unused */
typedef struct {
    uint64_t src;
    int64_t src_first, src_total, n_res;
    uint64_t dst16;
    int64_t dst_first;
    uint64_t win, delta, carry;
    int64_t carry_first;
    double scale, inc;
    int32_t src_held, dst_cap, index_step, nwin, carry_held, unused[3];
} w2l_resample_stream_entry;
typedef struct {
    int32_t stream, count;
    int64_t t0;
    double tr0;
    int32_t copy, unused;
} w2l_resample_block;
/* 1 <= nstreams <= 65535, 1 <= nblocks <= 1048576, num_table >= 1; every stream with non-NULL src, dst16, win and delta,
 * index_step >= 1, nwin >= 2 and counts >= 1; non-zero with w2l_last_error() set otherwise, or for a NULL / misaligned table, and
 * then nothing is launched */
int w2l_resample_stream(void* stream, const w2l_resample_stream_entry* streams_host, const w2l_resample_stream_entry* streams,
                        int nstreams, const w2l_resample_block* blocks, int nblocks, int num_table);

/* ---------------------------------------------------------------- SyncNet tail / losses */

/* x [N,x_cs] first C -> y [N,C] = x / max(||x||_2, 1e-12) */
int w2l_l2norm_rows(void* stream, int N, int C, const float* x, int x_cs, float* y);
/* a,v [N,C] -> cos[N] (eps 1e-8, F.cosine_similarity) and, if y != NULL, loss[0] = mean BCE(cos, y) */
int w2l_cosine_bce(void* stream, int N, int C, const float* a, const float* v, const float* y,
                   float* cos_out, float* loss_out);

/* p,y [N] -> loss[0] = mean( -(y*max(log p,-100) + (1-y)*max(log(1-p),-100)) )  (nn.BCELoss / F.binary_cross_entropy:
 * models/wav2lip.py:171, hq_wav2lip_train.py:249,253) */
int w2l_bce_mean(void* stream, int N, const float* p, const float* y, float* loss_out);

/* ---------------------------------------------------------------- training: conv weight gradient */

/* dweight (torch layout of `g`: [cout][cin][kh][kw], or [cin][cout][kh][kw] when transposed; device fp32, fully
 * overwritten) = d loss / d weight given the layer input x [N,H,W,x_cs] and the gradient dz [N,Ho,Wo,dz_cs] of the
 * convolution output (before BN / activation).  Both buffers must expose roundup(channels,4) readable channels per
 * pixel with ZERO pad channels, 16-byte aligned, channel strides multiples of 4.  Deterministic (fixed-order split-K). */
int w2l_conv_wgrad(const w2l_conv_geom* g, void* stream, int N, int H, int W, const float* x, int x_cs,
                   const float* dz, int dz_cs, float* dweight);

/* the same with the contraction arithmetic selectable (W2L_PREC_BF16: operands rounded to bf16 in the kernel, fp32
 * accumulate, bf16 matrix cores) */
int w2l_conv_wgrad_prec(const w2l_conv_geom* g, void* stream, int N, int H, int W, const float* x, int x_cs,
                        const float* dz, int dz_cs, float* dweight, int precision);

/* What a call of w2l_conv_wgrad_prec with these arguments would run, from the launcher's own planning code (the launch executes
 * the same plan).  Launches nothing, touches no device memory, needs no device.
 *   family: W2L_WGRAD_WINO (F(3x3,2x2) Winograd), W2L_WGRAD_DIRECT (the GEMM kernels) or W2L_WGRAD_SMALL (heads of <= 4 channels);
 *   cfg: tile configuration of the direct GEMM - 0..4 for W2L_PREC_F32, 0..5 for W2L_PREC_BF16 (2 * row size + [P width % 8 == 0]);
 *        -1 for the other families;  K: length of the reduction (P-grid pixels; Winograd: 2x2 tiles), kstep: its step (small head:
 *   pixel lanes), chunk: K per workgroup, ksplit = ceil(K / chunk) workgroups along K;  reduce_blocks: grid of the reduce kernel. */
#define W2L_WGRAD_WINO 0
#define W2L_WGRAD_DIRECT 1
#define W2L_WGRAD_SMALL 2
typedef struct w2l_wgrad_info {
    int family, cfg, ksplit, chunk, K, kstep, reduce_blocks;
} w2l_wgrad_info;
int w2l_conv_wgrad_resolve(const w2l_conv_geom* g, int N, int H, int W, int x_cs, int dz_cs, int precision, w2l_wgrad_info* out);
/* Tests / tuning: force tile configuration `cfg` of the fp32 direct GEMM (-1 = automatic; a configuration whose rows do not fit
 * the layer is ignored; any forced value keeps the Winograd kernel off) and switch the Winograd kernel on / off (wino = 1 / 0).
 * Process-wide; replaces what W2L_WGRAD_CFG / W2L_WINO_WGRAD gave. */
int w2l_conv_wgrad_set_cfg(int cfg, int wino);
/* The float-reciprocal index split of the weight-gradient kernels evaluated on the host, n times: which = 0 the direct GEMM's
 * (pixel -> image, row, column), 1 the Winograd kernel's (tile -> image, tile row, tile column); q[i], r[i] = what the kernel
 * computes for a[i] / d[i] with the reciprocal the launcher passes.  Test support. */
int w2l_wgrad_divmod_host(int which, int n, const int* a, const int* d, int* q, int* r);

/* ---------------------------------------------------------------- training in bf16 (BASELINE configs[3] / [4])
 * The bf16-STORAGE training path: activations, pre-BatchNorm conv outputs and their gradients live in HBM as NHWC bf16
 * (channel strides in ELEMENTS, multiples of 8, pad channels zero; 16-byte aligned pointers); master weights, weight
 * gradients, BatchNorm statistics / parameters, losses and Adam stay fp32.  Every contraction multiplies bf16 operands on
 * v_mfma_f32_32x32x16_bf16 and accumulates in fp32; every tensor is rounded to bf16 (RNE) exactly once, on its way out. */

/* A bf16-storage conv layer (forward of models/conv.py:8,24,36 and - on the transposed geometry over the same weight tensor -
 * its data gradient): y = act( conv(x, weight) * scale + shift (+ res) ), act = g->act.  `weight` is the fp32 master tensor in
 * torch layout; create / update pack it to bf16 (asynchronous on `stream`; call update after every optimiser step). */
typedef struct w2l_convb w2l_convb_t;
int w2l_convb_create(const w2l_conv_geom* g, const float* weight, void* stream, w2l_convb_t** out);
int w2l_convb_update(w2l_convb_t* c, const float* weight, void* stream);
/* The same re-pack for n layers in ONE launch (what optimizer.step() in wav2lip_train.py:231 invalidates:
 * every layer's slabs).  weights[i] is the fp32 master tensor of handles[i]; the device-side tables are cached per (handle,
 * weight pointer) list, so steady-state training steps cost one kernel launch.  Bytes written == n calls of w2l_convb_update. */
int w2l_convb_update_many(int n, w2l_convb_t* const* handles, const float* const* weights, void* stream);
int w2l_convb_destroy(w2l_convb_t* c);
/* x bf16 [N,H,W,x_cs], y bf16 [N,Ho,Wo,y_cs] (channels [0, roundup(cout,8)) of each pixel written, pad channels zero), res
 * optional bf16 [N,Ho,Wo,res_cs] (may alias y: accumulate); scale / shift fp32 [cout] device vectors or NULL (1 / 0).
 * ksplit_force: 0 = automatic (a function of the shape), >= 1 forces the split-K factor (tests). */
int w2l_convb_forward(const w2l_convb_t* c, void* stream, int N, int H, int W, const void* x, int x_cs, void* y, int y_cs,
                      const void* res, int res_cs, const float* scale, const float* shift, int ksplit_force);
/* The conv in front of a batch-statistics BatchNorm (models/conv.py:8-10,36-40 in train mode): z = conv(x) + bias (bf16, no
 * activation) AND the statistics of z in one call - mean, rstd, scale = gamma*rstd, shift = beta - mean*scale (each
 * roundup(cout,8) entries, pad entries 0) and the running-stat update, as w2l_bn_train_stats_bf16 computes them.  The sums are
 * taken from the fp32 accumulators in the conv epilogue (per-wave column partials, fixed-order reduce) whenever the launch has
 * no split-K; otherwise the stand-alone reduction over z runs.  Saves one pass over z per layer. */
int w2l_convb_forward_bn(const w2l_convb_t* c, void* stream, int N, int H, int W, const void* x, int x_cs, void* z, int z_cs,
                         const float* bias, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, float* mean, float* rstd, float* scale, float* shift);
/* A data-gradient launch whose output IS the dy of a batch-statistics BatchNorm block (the block in front of this layer in
 * models/conv.py chains: wav2lip_train.py:225 loss.backward() through Conv2d -> Conv2d): y = conv(x) (+ res) in bf16 as
 * w2l_convb_forward writes it AND the two column sums BatchNorm's backward needs over that block - dbeta[c] = sum g,
 * dgamma[c] = sum g * zhat with g = y * act'(block output), zhat = (bz - mean) * rstd - taken in the conv epilogue from the
 * bf16-ROUNDED outputs (what w2l_bn_train_bwd_apply_bf16 then re-reads), per-wave column partials, fixed-order reduce.  bz:
 * the block's pre-BatchNorm conv output [N,Ho,Wo,bz_cs]; by: its output, or NULL for a ReLU block without residual (sign
 * recomputed as bz*bscale + bshift > 0); bact its activation (none / ReLU / LeakyReLU).  *fused_out = 1 when the sums were
 * written (C = roundup(cout,8) entries each, pad entries 0); 0 when the launch split K - y is written all the same and the
 * caller runs w2l_bn_train_bwd_bf16.  Saves the stand-alone reduction's pass over dy, z (and y) per block.
 * bact | W2L_BNBWD_STORE_MASKED (ReLU blocks only): when the sums are fused (*fused_out = 1) the launch stores g = dy * [block
 * output > 0] - bit for bit the bf16 dy or zero - INSTEAD of dy.  The block's own backward pass is then
 * w2l_bn_train_bwd_apply_bf16(dy = that tensor, y = NULL, act = W2L_ACT_NONE, g_out = NULL): it reads neither the block's output
 * for the mask again nor writes g (the residual path's operand is already in place): two tensor passes less per residual block.
 * With *fused_out = 0 (split-K) plain dy was stored. */
#define W2L_BNBWD_STORE_MASKED 0x100
int w2l_convb_forward_bnbwd(const w2l_convb_t* c, void* stream, int N, int H, int W, const void* x, int x_cs, void* y, int y_cs,
                            const void* res, int res_cs, const void* bz, int bz_cs, const void* by, int by_cs, int bact,
                            const float* mean, const float* rstd, const float* bscale, const float* bshift, float* dgamma,
                            float* dbeta, int* fused_out);
/* The same for an activation block WITHOUT BatchNorm (models/conv.py:22-31 `nonorm_Conv2d`: conv + LeakyReLU; the discriminator of
 * hq_wav2lip_train.py:246-256): the data-gradient launch that completes the block's dy stores dz = dy * act'(by) directly - the
 * bf16-ROUNDED dy times 1 / slope, rounded again by the store: bit for bit what w2l_act_bwd_bf16 computes from the stored dy - so
 * that the block's own backward pass needs no elementwise launch at all.  by: the block's OUTPUT; bact: ReLU or LeakyReLU.
 * dbias (optional, roundup(cout,8) floats): the column sums of the stored dz = the gradient of the block's conv bias
 * (sum over pixels), from per-wave partials of the same epilogue: the stand-alone w2l_col_sum_bf16 pass over dz is not needed.
 * *fused_out = 0 when the launch split K or ran on a special-case kernel: plain dy was stored, dbias was not written, and the
 * caller runs w2l_act_bwd_bf16 (and w2l_col_sum_bf16). */
int w2l_convb_forward_actbwd(const w2l_convb_t* c, void* stream, int N, int H, int W, const void* x, int x_cs, void* y, int y_cs,
                             const void* res, int res_cs, const void* by, int by_cs, int bact, float* dbias, int* fused_out);
/* Fuse a following 1x1 convolution + activation into the layer (the generator's output block on the bf16-storage inference path,
 * models/wav2lip.py:83-85: Conv2d(80,32,3)+BN+ReLU -> nn.Conv2d(32,head_c,1) -> Sigmoid), the bf16 form of w2l_conv_attach_head.
 * The layer must be a 3x3 stride-1 pad-1 conv with cin % 16 == 0 and 32 couts; `weight` is its fp32 master tensor again (the head
 * kernel keeps its own bf16 copy, re-packed by w2l_convb_update / _update_many), head_weight [head_c][32], head_bias [head_c] or
 * NULL: device fp32, head_c <= 4.  Such a layer runs through w2l_convb_forward_head only. */
int w2l_convb_attach_head(w2l_convb_t* c, const float* weight, const float* head_weight, const float* head_bias, int head_c,
                          int head_act, void* stream);
/* x bf16 [N,H,W,x_cs] (16-byte aligned, x_cs % 8 == 0); scale / shift fp32 [32] (the folded BatchNorm, applied to the fp32
 * accumulators).  The head output v (fp32, never rounded to bf16) goes to frames u8 [N,H,W,head_c] = (uint8)(v*255.f), the
 * truncation of w2l_frames_to_u8, and - if y32 != NULL - to y32 fp32 [N,H,W,y32_cs] as well. */
int w2l_convb_forward_head(const w2l_convb_t* c, void* stream, int N, int H, int W, const void* x, int x_cs, uint8_t* frames,
                           float* y32, int y32_cs, const float* scale, const float* shift);
/* tile override for tests / tuning: -1 = automatic */
int w2l_convb_set_tile(w2l_convb_t* c, int tile);
int w2l_convb_num_tiles(void);
/* The kernel a launch of this layer over [N,H,W] (has_res: with a residual) resolves to - what w2l_convb_forward with
 * ksplit_force 0, a w2l_plan_add_convb item or, for a layer with a fused head, w2l_convb_forward_head would run: the function
 * of the shape the launcher itself calls before it launches, over dense strides.  Launches nothing, touches no device memory.
 *   *family: W2L_CONVB_IGEMM (*tile = tile id, *ksplit = split-K), W2L_CONVB_STEM (*tile = the stem kernel's layer family 1..4),
 *            W2L_CONVB_BOX64, W2L_CONVB_TP2B or W2L_CONVB_HEAD (the fused output block); *tile = -1, *ksplit = 1 where not given. */
#define W2L_CONVB_IGEMM 0
#define W2L_CONVB_STEM 1
#define W2L_CONVB_BOX64 2
#define W2L_CONVB_TP2B 3
#define W2L_CONVB_HEAD 4
int w2l_convb_resolve(const w2l_convb_t* c, int N, int H, int W, int has_res, int* family, int* tile, int* ksplit);
/* The same answer from the geometry alone (no layer handle, no device, automatic tile), and *flops: the FLOPs the matrix cores
 * execute for that launch (padded tiles and K), as w2l_plan_executed_flops and the w2l_flops_begin counter report them. */
int w2l_convb_resolve_geom(const w2l_conv_geom* g, int N, int H, int W, int has_res, int* family, int* tile, int* ksplit,
                           long long* flops);

/* Weight gradient on the bf16-storage path: dweight (fp32, torch layout of `g`, fully overwritten) from the layer input
 * x bf16 [N,H,W,x_cs] and the gradient dz bf16 [N,Ho,Wo,dz_cs] of the convolution output.  Same contract as w2l_conv_wgrad
 * otherwise (zero pad channels, deterministic fixed-order split-K). */
int w2l_conv_wgrad_bf16(const w2l_conv_geom* g, void* stream, int N, int H, int W, const void* x, int x_cs,
                        const void* dz, int dz_cs, float* dweight);
/* The plan of that call, from the launcher's own planning code; launches nothing, needs no device.  A workgroup walks
 * boxes_per_split boxes (the last split: the rest of nboxes) of ni images x bh x bw P pixels; ntg tap groups of tg taps, ncq
 * 64-channel Q slices, mt / qp 32-channel planes of P / Q. */
typedef struct w2l_wgrad_bf16_info {
    int ni, bh, bw, nboxes, splits, boxes_per_split, ntg, tg, ncq, mt, qp;
} w2l_wgrad_bf16_info;
int w2l_conv_wgrad_bf16_resolve(const w2l_conv_geom* g, int N, int H, int W, int x_cs, int dz_cs, w2l_wgrad_bf16_info* out);

/* BatchNorm (batch statistics) / activation / residual passes over bf16 tensors: the bf16 twins of the fp32 entry points
 * below (same arithmetic in fp32 / fp64, 8 channels = 16 bytes per thread and row).  C = channels of the row view, a multiple
 * of 8 (pad channels included, zero in the tensors); Cvalid = channels that exist.  Per-channel OUTPUT vectors (mean, rstd,
 * scale, shift, dgamma, dbeta, column sums) have C entries - the pad entries are written as 0 so that the elementwise passes
 * can load them as vectors; per-channel INPUT parameters (gamma, beta, running stats) have Cvalid entries. */
int w2l_bn_train_stats_bf16(void* stream, long long rows, int C, int Cvalid, const void* z, int z_cs, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                            float* rstd, float* scale, float* shift);
int w2l_affine_act_bf16(void* stream, long long rows, int C, const void* z, int z_cs, const float* scale, const float* shift,
                        const void* res, int res_cs, int act, void* y, int y_cs);
/* y may be NULL for a ReLU block WITHOUT residual when `shift` (the forward's beta - mean*gamma*rstd, C entries) is given: the
 * activation mask is then recomputed as z*scale + shift > 0 - the forward's own expression - and the pass reads one tensor less */
int w2l_bn_train_bwd_bf16(void* stream, long long rows, int C, int Cvalid, const void* dy, int dy_cs, const void* y, int y_cs,
                          const void* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                          const float* shift, float* dgamma, float* dbeta, void* dz, int dz_cs, void* g_out, int g_cs);
/* the elementwise half of w2l_bn_train_bwd_bf16 alone, with the column sums (dgamma, dbeta: C entries) as INPUTS - after
 * w2l_convb_forward_bnbwd has produced them in the epilogue of the launch that wrote dy.  act = W2L_ACT_NONE with y = NULL: `dy`
 * already is the masked gradient g (W2L_BNBWD_STORE_MASKED). */
int w2l_bn_train_bwd_apply_bf16(void* stream, long long rows, int C, const void* dy, int dy_cs, const void* y, int y_cs,
                                const void* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                                const float* shift, const float* dgamma, const float* dbeta, void* dz, int dz_cs, void* g_out,
                                int g_cs);
int w2l_act_bwd_bf16(void* stream, long long rows, int C, const void* dy, int dy_cs, const void* y, int y_cs, int act,
                     const float* scale, void* dz, int dz_cs, void* g_out, int g_cs);
int w2l_add_rows_bf16(void* stream, long long rows, int C, const void* a, int a_cs, const void* b, int b_cs, void* out, int out_cs);
int w2l_col_sum_bf16(void* stream, long long rows, int C, const void* x, int x_cs, float* out);
/* The THIN 1x1 convolution (cin <= 32, cout <= 4) over [npix] rows - the generator's output layer nn.Conv2d(32, 3, 1) + Sigmoid
 * (models/wav2lip.py:83-85) in a training step: HBM-bound row kernels instead of a 128x32 GEMM tile that multiplies 29/32 padding.
 * w: fp32 [cout][cin] (the torch weight of a 1x1 conv), rounded to bf16 on the way in as the GEMM path rounds it; fp32 sums.
 * forward: y[p][o] = act(sum_c x[p][c] w[o][c] + bias[o]), 8 channels of y written (pad zero);
 * dgrad:   dx[p][c] = sum_o dz[p][o] w[o][c] (+ res[p][c]; res may alias dx), roundup(cin,8) channels written;
 * wgrad:   dweight[o][c] = sum_p dz[p][o] x[p][c] and (dbias != NULL) dbias[o] = sum_p dz[p][o], fp32, fixed summation order. */
int w2l_thin1x1_forward_bf16(void* stream, long long npix, int cin, int cout, const void* x, int x_cs, const float* w,
                             const float* bias, int act, void* y, int y_cs);
int w2l_thin1x1_dgrad_bf16(void* stream, long long npix, int cin, int cout, const void* dz, int dz_cs, const float* w,
                           const void* res, int res_cs, void* dx, int dx_cs);
int w2l_thin1x1_wgrad_bf16(void* stream, long long npix, int cin, int cout, const void* x, int x_cs, const void* dz, int dz_cs,
                           float* dweight, float* dbias);
/* workgroups (= partial rows) w2l_thin1x1_wgrad_bf16 launches for npix pixels: the launcher's own rule */
int w2l_thin1x1_wgrad_blocks(long long npix);
/* graph boundary: x fp32 [N,C,H,W] -> y bf16 [N,H,W,y_cs] (channels [C, c_zero_to) zero-filled) and back */
int w2l_nchw_to_nhwc_bf16(void* stream, int N, int C, int H, int W, const float* x, void* y, int y_cs, int c_zero_to);
int w2l_nhwc_bf16_to_nchw(void* stream, int N, int C, int H, int W, const void* x, int x_cs, float* y);

/* ---------------------------------------------------------------- training: BatchNorm (batch statistics), activations
 * All tensors below are NHWC row views [rows][cs] with C valid channels; C %% 4 == 0, cs %% 4 == 0, 16-byte aligned. */

/* Per-channel batch statistics of z: mean, rstd = 1/sqrt(biased var + eps), and the affine form used by the forward
 * (scale = gamma*rstd, shift = beta - mean*scale).  running_mean / running_var (NULL = skip) are updated in place with
 * `momentum` and the unbiased variance, as nn.BatchNorm2d does in train mode. */
int w2l_bn_train_stats(void* stream, long long rows, int C, const float* z, int z_cs, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* mean, float* rstd, float* scale, float* shift);
/* y = act( z*scale + shift (+ res) ) */
int w2l_affine_act(void* stream, long long rows, int C, const float* z, int z_cs, const float* scale,
                   const float* shift, const float* res, int res_cs, int act, float* y, int y_cs);
/* Backward of y = act( gamma*(z-mean)*rstd + beta (+ res) ):  g = dy * act'(y);  dbeta = sum g;  dgamma = sum g*zhat;
 * dz = scale*(g - dbeta/rows - zhat*dgamma/rows) with scale = gamma*rstd.  g_out (NULL = skip; may alias dy) receives g,
 * which is also the gradient of the residual input. */
int w2l_bn_train_bwd(void* stream, long long rows, int C, const float* dy, int dy_cs, const float* y, int y_cs,
                     const float* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                     float* dgamma, float* dbeta, float* dz, int dz_cs, float* g_out, int g_cs);
/* g = dy * act'(y) (y may be NULL for W2L_ACT_NONE);  dz = g * scale[c] (scale NULL = 1: eval-mode BN folds to a
 * per-channel scale);  g_out as above. */
int w2l_act_bwd(void* stream, long long rows, int C, const float* dy, int dy_cs, const float* y, int y_cs, int act,
                const float* scale, float* dz, int dz_cs, float* g_out, int g_cs);
/* out = a + b (out may alias either) */
int w2l_add_rows(void* stream, long long rows, int C, const float* a, int a_cs, const float* b, int b_cs, float* out,
                 int out_cs);
/* out[c] = sum over rows of x[row][c]  (bias gradient) */
int w2l_col_sum(void* stream, long long rows, int C, const float* x, int x_cs, float* out);

/* ---------------------------------------------------------------- training: losses (gout = upstream gradient, a device
 * scalar, NULL = 1) */
int w2l_l1_mean(void* stream, long long n, const float* a, const float* b, float* loss_out);
int w2l_l1_bwd(void* stream, long long n, const float* a, const float* b, const float* gout, float* da);
int w2l_cosine_bce_bwd(void* stream, int N, int C, const float* a, const float* v, const float* y, const float* gout,
                       float* da, float* dv);
int w2l_l2norm_bwd(void* stream, int N, int C, const float* x, int x_cs, const float* dy, float* dx, int dx_cs);
int w2l_bce_bwd(void* stream, int N, const float* p, const float* y, const float* gout, float* dp);

/* ---------------------------------------------------------------- evaluation: LSE-style sync distance table
 * out [T][2*vshift+1]: out[i][j] = || f1[i] - pad(f2)[i+j] + 1e-6 ||_2 with f2 zero-padded by vshift rows on both sides
 * (calc_pdist, evaluation/scores_LSE/SyncNetInstance_calc_scores.py:19-31); f1, f2 [T][C] fp32. */
int w2l_shifted_pdist(void* stream, int T, int C, int vshift, const float* f1, const float* f2, float* out);

/* ---------------------------------------------------------------- evaluation: scoring a directory of clips
 * (evaluation/scores_LSE/calculate_scores_LRS.py:28-50 calls, per video, SyncNetInstance_calc_scores.py:105-137: windows of 5
 * frames and of the matching audio features through the two encoders, calc_pdist (:19-31), mean over the windows, min, median.)
 * Windows are independent given eval-mode weights, so windows of different clips share a SyncNet batch: a row names its own
 * clip.  Tables live in device memory.
 *
 * w2l_sync_row, 32 bytes, alignment 16: one window (wav2lip_train.py:80,192-195 layout)
 *   byte  0  uint64 frames  device address of the window's first frame: five consecutive face crops, u8 [5][S][S][3]
 *   byte  8  uint64 mel     device address of the clip's spectrogram, fp32 [80][T]
 *   byte 16  int32  T       its number of columns
 *   byte 20  int32  start   the window is columns [start, start+16) (columns outside [0,T) read as 0)
 *   byte 24  int32  pad[2]  unused (keeps consecutive rows 16-byte aligned)
 * w2l_lse_segment, 8 bytes, alignment 8: one clip's rows of the two embedding arrays
 *   byte  0  int32  row0    its first row
 *   byte  4  int32  n       its number of rows */
typedef struct {
    uint64_t frames, mel;
    int32_t T, start;
    int32_t pad[2];
} w2l_sync_row;
typedef struct {
    int32_t row0, n;
} w2l_lse_segment;

/* Both inputs of a SyncNet plan for B windows, written whole (pad channels included: the result does not depend on what the
 * buffers held):
 *   face_in fp32 [B][S/2][S][face_cs]:  [b][y][x][3*t+c] = float(frame[t][S/2+y][x][c]) / 255.f (correctly rounded: bit-equal to
 *                                       numpy u8.astype(float32) / float32(255)), channels 15 .. face_cs-1 = 0
 *   mel_in  fp32 [B][80][16][mel_cs]:   [b][r][k][0] = mel[r*T + start + k], channels 1 .. mel_cs-1 = 0
 * face_cs >= 16 and mel_cs >= 4, both multiples of 4; outputs 16-byte aligned; 1 <= B <= 65535. */
int w2l_sync_window_rows(void* stream, int B, const w2l_sync_row* rows, int S, float* face_in, int face_cs, float* mel_in,
                         int mel_cs);
/* The same for the bf16-storage plan: face_in / mel_in are bf16, every value the fp32 one above rounded once (round to nearest
 * even), pad channels written as zeros.  8 channels (16 bytes) per store: face_cs >= 16 and mel_cs >= 8, both multiples of 8;
 * outputs 16-byte aligned; 1 <= B <= 65535. */
int w2l_sync_window_rows_bf16(void* stream, int B, const w2l_sync_row* rows, int S, void* face_in, int face_cs, void* mel_in,
                              int mel_cs);
/* The tail of the bf16-storage SyncNet plan, both encoders in one launch: row b of audio_x bf16 [B][audio_cs] -> row b of
 * audio_out fp32 [B][C] (contiguous), face_x bf16 [B][face_cs] -> face_out likewise, y = x / max(||x||_2, 1e-12) over the first C
 * channels (the others are not read), the sum of squares in fp32.  C and both strides (>= C) are multiples of 8; all four
 * pointers 16-byte aligned; B >= 1.  A caller that fills rows [offset, offset+B) of an arena passes arena + offset*C. */
int w2l_sync_embeddings_bf16(void* stream, int B, int C, const void* audio_x, int audio_cs, const void* face_x, int face_cs,
                             float* audio_out, float* face_out);
/* SyncNetInstance_calc_scores.py:129-137 for n_seg clips in one launch.  face_emb, audio_emb fp32 [rows][C]; segment s owns rows
 * [row0, row0+n) of both.  With win = 2*vshift+1 and dist(i, j) the entry of w2l_shifted_pdist run on the segment alone (zero
 * padding at the segment's own ends; no row of another segment is read; the same arithmetic, bit for bit):
 *   mdist  fp32 [n_seg][win]:  mdist[s][j] = mean over i of dist(i, j), summed in fp64 in row order, rounded to fp32 once
 *   scores fp32 [n_seg][4]:    (min_j mdist, median_j mdist - min, vshift - argmin, n); the argmin is the lowest j among equal
 *                              minima, the median the element of rank (win-1)/2 (torch.median's lower median)
 * n_seg >= 1, C >= 1, 0 <= vshift <= 127 (win <= 255: one workgroup per segment).  A segment with n < 1 reads nothing and gets
 * NaN scores with n = 0. */
int w2l_lse_score_segments(void* stream, int n_seg, const w2l_lse_segment* segs, int C, int vshift, const float* face_emb,
                           const float* audio_emb, float* mdist, float* scores);

/* ---------------------------------------------------------------- training: fused multi-tensor Adam */
typedef struct w2l_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;
} w2l_adam_tensor;
typedef struct w2l_adam w2l_adam_t;
/* sizes_host[ntensors]: element counts (host array); builds the block -> (tensor, chunk) table once */
int w2l_adam_create(int ntensors, const long long* sizes_host, w2l_adam_t** out);
int w2l_adam_destroy(w2l_adam_t* h);
/* One optimiser step over all tensors in ONE launch (torch.optim.Adam semantics, amsgrad off; step counts from 1).
 * tensors_host[ntensors] (host array of device pointers; gradient tensors may move between steps) must stay valid
 * until the stream has consumed the copy. */
int w2l_adam_step(w2l_adam_t* h, void* stream, const w2l_adam_tensor* tensors_host, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step);

/* ---------------------------------------------------------------- plans (a recorded sequence of launches) */

typedef struct w2l_plan w2l_plan_t;
int w2l_plan_create(w2l_plan_t** out);
int w2l_plan_destroy(w2l_plan_t* p);
/* record one conv launch with fixed buffers/shapes; replayed in order by w2l_plan_run */
int w2l_plan_add_conv(w2l_plan_t* p, const w2l_conv_t* c, int N, int H, int W, const float* x, int x_cs,
                      float* y, int y_cs, const float* res, int res_cs);
/* record one bf16-storage launch (w2l_convb_forward with ksplit_force 0) with its per-item scale / shift; validated when recorded.
 * Its configuration comes from the shape (the convb rules): w2l_plan_autotune skips it, w2l_plan_get_config reports (-1, 1) and
 * w2l_plan_set_config accepts only that; w2l_plan_executed_flops reports configuration id -1. */
int w2l_plan_add_convb(w2l_plan_t* p, const w2l_convb_t* c, int N, int H, int W, const void* x, int x_cs, void* y, int y_cs,
                       const void* res, int res_cs, const float* scale, const float* shift);
/* record one w2l_convb_forward_head launch (a layer with w2l_convb_attach_head), same rules */
int w2l_plan_add_convb_head(w2l_plan_t* p, const w2l_convb_t* c, int N, int H, int W, const void* x, int x_cs, uint8_t* frames,
                            float* y32, int y32_cs, const float* scale, const float* shift);
/* append a copy of launch `index` of `src` (same layer, buffers and configuration) to `dst`: sub-plans for multi-stream runs */
int w2l_plan_copy_item(w2l_plan_t* dst, const w2l_plan_t* src, int index);
int w2l_plan_run(const w2l_plan_t* p, void* stream);
int w2l_plan_size(const w2l_plan_t* p);
/* OPT-IN stopwatch autotune: time every (tile configuration, split-K factor) candidate of every recorded launch on its real
 * buffers (reps timed runs each, HIP events on `stream`, synchronises), keep the fastest for w2l_plan_run and record it in
 * the tune table below.  A stopwatch choice differs from box to box and run to run, and with it the summation order of the
 * layer: the default path (no autotune) is the table, then a heuristic - both functions of the shape only. */
int w2l_plan_autotune(w2l_plan_t* p, void* stream, int reps);
int w2l_plan_get_config(const w2l_plan_t* p, int index, int* tile, int* ksplit);
int w2l_plan_set_config(w2l_plan_t* p, int index, int tile, int ksplit);   /* tile -1 = heuristic */
/* FLOPs the matrix cores EXECUTE per recorded launch with its current configuration (padded tiles and K; Winograd layers:
 * 16 products per 2x2 output tile per (cin, cout) instead of 36): flops_out[w2l_plan_size].  Launches nothing.  This is the
 * numerator of bench.py's roofline fraction (the nominal direct-convolution count is w2l_conv_macs).  config_out (optional,
 * [w2l_plan_size][2]) receives the (configuration id, split-K) each launch resolves to - explicit, tune table or heuristic;
 * ids below w2l_conv_num_igemm_tiles() are implicit-GEMM tiles, the rest Winograd configurations. */
int w2l_plan_executed_flops(const w2l_plan_t* p, long long* flops_out, int* config_out);
int w2l_conv_num_igemm_tiles(void);
/* Executed-FLOP counter for whole training steps (tools/train_bench.py): between w2l_flops_begin() and w2l_flops_end() every
 * conv / data-gradient / weight-gradient launch of the process (any thread: backward() runs on torch's autograd thread) ALSO adds the multiply-add work its matrix cores execute
 * (padded tiles and K, 16 or 9 instead of 36 products on Winograd launches) to a counter; w2l_flops_end returns the total and,
 * if by_family != NULL, by_family[8]: 0 fp32 conv, 1 fp32 weight gradient (direct), 2 fp32 Winograd weight gradient, 3 / 4 the
 * round-2 bf16-contraction conv / weight gradient, 5 / 6 the bf16-storage conv / weight gradient, 7 non-MFMA head reductions. */
int w2l_flops_begin(void);
long long w2l_flops_end(long long* by_family);
/* Shader-clock probe (measurement aid of bench.py, no reference counterpart): one wave spins `spin_us` microseconds on `stream`
 * and writes out2_dev[0] = shader-clock ticks (s_memtime), out2_dev[1] = 100 MHz reference ticks (s_memrealtime) of the spin;
 * MHz = 100 * out[0] / out[1].  Run on a side stream while a workload runs: the clock the chip sustains under that workload. */
int w2l_clock_probe(void* stream, int spin_us, unsigned long long* out2_dev);
/* kernel family of a configuration id: 0 = conv_igemm_f32_kernel, 1 = conv_wino_f32_kernel, 2 = conv_wino2_f32_kernel,
 * (conv_wino2.hip: ids 8, 9 and the quarter-split shape, id 12), 3 = conv_tp2_f32_kernel (stride-2 transposed 3x3, all four
 * phases in one workgroup), 4 = conv_wino4_f32_kernel (Winograd F(4x4,3x3)), 5 = the split-operand implicit GEMM (ids 13..18 =
 * the implicit-GEMM tiles 0..5 again, W2L_PREC_F32 layers only: every fp32 operand enters the bf16 matrix cores as the exact sum of
 * three bf16 pieces, six piece products per product, fp32 accumulate - an fp32 result with the fp32 kernels' error, not bitwise
 * theirs; the committed table gives it ten batch-128 generator launches, W2L_SPLIT=0 puts their fp32-pipe entries back), 6 = the
 * same arithmetic inside Winograd F(2x2,3x3) (conv_wino2s_kernel, id 19), 7 = inside the fused-phase stride-2 transposed kernel
 * (conv_tp2s_kernel, id 20), 8 = the generator's 7x7 first layer with the region staged and split once (conv_stem7s_kernel, id 21),
 * 9 = the direct 3x3 kernel for 32-cout layers with the optional fused 1x1 head (conv_k3s_kernel, id 22); -1 = bad id.  Ids are append-only across library versions. */
int w2l_conv_config_family(int id);
/* Switch kernel families off (bit f of `mask` = family f of w2l_conv_config_family; family 0, the implicit GEMM, cannot be
 * excluded): w2l_plan_autotune skips their ids and a table / forced id of an excluded family falls through to the next rule.
 * mask < 1024.  mask 16 (= no conv_wino4) is how the "exact" launch table is built and run: F(4x4,3x3) carries about twice the rounding
 * error of F(2x2,3x3) (7.7e-7 vs 4.2e-7 pixel L-inf against the reference). */
int w2l_conv_exclude_families(int mask);
/* The implicit-GEMM kernels' workgroup -> (phase, M-tile, cout-tile) map (measurement / test aid, no reference counterpart; host
 * code, runs without a GPU): out[3 * i ..] = (phase, tile_m, tile_n) of the i-th workgroup in dispatch order for a grid of
 * tiles_m * tiles_n x nphase workgroups (every K-split repeats it); workgroup i runs on XCD i % 8.  order 0 = phase-major, cout-tiles
 * fastest inside a phase; 1 = phase-major, cout-tile slowest inside a phase (weight-heavy layers: an XCD fetches its 1/8 of the
 * weights once); 2 = groups of order_r M-tiles phase by phase (a stride-2 transposed layer's four phases re-read their input out of an
 * XCD's L2 instead of HBM).  The launcher chooses per shape. */
int w2l_igemm_block_order(int order, int order_r, int tiles_m, int tiles_n, int nphase, int* out);
/* How configuration 11 (Winograd F(4x4,3x3)) packs its 32 tile slots for N images of H x W (test aid, host code, runs without a
 * GPU; a function of the shape alone).  out[8] = {form, blocks, r, c, ni, pitch, pad, cells}: form 0 = rectangles of r x c tiles in
 * each of ni images (pad = the image stride in plane cells), form 1 = runs of r consecutive (image, tile row) units at the full
 * tile width c, crossing image boundaries (pad = extra plane cells in front of every segment after the first); blocks = work items
 * per 64-cout tile, pitch = plane cells per staged raw row, cells = cells per raw plane. */
int w2l_wino4_block_plan(int N, int H, int W, int* out);
/* The block of output a work item of a GROUPED kernel family covers for N images of H x W input (test aid, host code, runs without
 * a GPU; a function of the shape alone, the launcher's own choice): out[3] = {bh, bw, ni} - bh x bw tiles of 2 x 2 output pixels
 * (conv_wino2 ids 8, 9, 12, conv_wino2s) or input pixels (conv_tp2, conv_tp2s) or output pixels (conv_k3s) in each of ni images;
 * ceil(N / ni) image groups, the last of which runs past the batch when N % ni != 0.  Error for an id of another family
 * (conv_wino4 has w2l_wino4_block_plan; the implicit GEMM and conv_wino walk a flat pixel / tile index, conv_stem7s one image). */
int w2l_conv_block_plan(int id, int N, int H, int W, int* out);
/* time each recorded launch with HIP events on `stream` (reps runs, averaged): ms_out[w2l_plan_size] */
int w2l_plan_profile(const w2l_plan_t* p, void* stream, int reps, float* ms_out);

/* ---------------------------------------------------------------- tune table (shape -> launch configuration)
 * A conv launch without an explicit configuration looks its shape up here; a miss runs the library's heuristic.  Both are
 * pure functions of the shape, so results are bit-reproducible across runs and boxes (the reference's torch ops are
 * deterministic on CPU; a stopwatch-tuned path is not).  Key = W2L_TUNE_KEY_INTS ints: transposed, cin, cout, kh, kw, sh,
 * sw, ph, pw, oph, opw, precision (W2L_PREC_*), has_residual, head_c, N, H, W.  The host side loads the committed
 * wav2lip_amd/tune_table.json at start-up (tools/make_tune_table.py regenerates it on a GPU box). */
#define W2L_TUNE_KEY_INTS 17
int w2l_tune_key_ints(void);
int w2l_tune_set(const int* key, int tile, int ksplit);
/* 1 if configuration id `tile` can run a launch with this key (geometry / precision / residual / head eligibility of the
 * kernel family behind the id), 0 if such a launch would fall through to the heuristic: table writers and the table test use it */
int w2l_tune_entry_applicable(const int* key, int tile);
int w2l_tune_clear(void);
int w2l_tune_count(void);
/* out[cap_entries][W2L_TUNE_KEY_INTS + 2] = key, tile, ksplit per entry; returns the number of entries written */
int w2l_tune_export(int* out, int cap_entries);

#ifdef __cplusplus
}
#endif
#endif /* W2L_HIP_H */
