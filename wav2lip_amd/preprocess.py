"""The dataset preparation step of the reference (preprocess.py) on the HIP face detector: every frame of every clip under
`--data_root/<dir>/<vid>.{mp4,avi}` goes through S3FD in batches of `--batch_size`, the first detection of a frame is cut out of
it with no pads and no smoothing and written as `--preprocessed_root/<dir>/<vid>/<i>.jpg` (i counts every frame; a frame without
a face writes nothing, so the ids have gaps), and the clip's audio track is written next to the crops as `audio.wav`.  That is
the layout `trainer.main_*` and `data.ClipStore.from_directory` read.

    python -m wav2lip_amd.preprocess --data_root LRS2/main --preprocessed_root lrs2_preprocessed/ [--batch_size 32]
    python -m torch.distributed.run --nproc-per-node 8 -m wav2lip_amd.preprocess --ngpu 8 --data_root ... --preprocessed_root ...

Per frame batch: the detector graph (fp32, or bf16 storage with `--face_det_precision bf16`), the gate + NMS and the rect rule run
on the device and one [B][5] int32 array comes back (FaceAlignment.get_detections_for_batch).  The ragged last batch of a clip is
padded with copies of its last frame, so that every batch of a clip size runs the same cached detector graph.  The JPEG encoding
(what cv2.imwrite does by default: quality 95, 4:2:0) runs by default on the host, in a small thread pool that overlaps the next
batch's detection (PIL releases the GIL while it encodes).  With `--jpeg device` the batch is uploaded once, the detector reads it
from device memory and the crops are encoded there, out of the same tensor (jpeg.CropEncoder, w2l_jpeg_encode_rows): only the
files' bytes come back, and the pool's job is the file write.  Both write the same bytes.

Differences from the reference, all on the file-format side: video is read with container.read_avi (uncompressed 24-bit
BGR AVI with PCM16 audio); an .mp4 cannot be decoded here and is reported and skipped like any failing clip.  The reference's
ffmpeg `-i <video> -strict -2 audio.wav` keeps the source's rate and channels as PCM16; the AVI's PCM16 stream is written
unchanged as a WAV with the stdlib `wave` module.  Multi-GPU is one process per GPU (torch.distributed.run), not threads: rank r
takes the clips i with i % WORLD_SIZE == r, as the reference deals jobs to its GPUs, and the ranks meet only at a final barrier.
"""
import argparse
import os
import traceback
import wave
from concurrent.futures import ThreadPoolExecutor, wait
from glob import glob
from os import path

import numpy as np

from . import container

JPEG_WORKERS = 4          # host encoder threads; the detector owns the device, so a few threads keep up with it
JPEG_QUALITY = 95         # cv2.imwrite's default IMWRITE_JPEG_QUALITY
JPEG_SUBSAMPLING = 2      # PIL's code for 4:2:0, libjpeg's default that cv2 keeps


def build_parser():
    """preprocess.py:21-26: the reference's flags, names, types and defaults, plus `--face_det_precision` (as inference has)"""
    parser = argparse.ArgumentParser()
    parser.add_argument('--ngpu', help='Number of GPUs across which to run in parallel', default=1, type=int)
    parser.add_argument('--batch_size', help='Single GPU Face detection batch size', default=32, type=int)
    parser.add_argument("--data_root", help="Root folder of the LRS2 dataset", required=True)
    parser.add_argument("--preprocessed_root", help="Root folder of the preprocessed dataset", required=True)
    parser.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                        help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage (faster; boxes move '
                             'by about what bf16 rounding alone moves them)')
    return parser


def build_main_parser():
    """what the command line parses: `build_parser` plus `--face_det_scale K` (`inference.add_det_scale_flag`): the detector sees
    every frame at 1/K of its size, the crops are cut from the full-resolution frame at the rects mapped back; and `--jpeg`, where
    the crops are encoded"""
    from .inference import add_det_scale_flag
    p = build_parser()
    add_det_scale_flag(p)
    p.add_argument('--jpeg', default='host', choices=['host', 'device'],
                   help='Where the face crops are JPEG-encoded: host (default, a PIL thread pool) or device (a HIP kernel on the '
                        'frames the detector has just read; the same bytes)')
    return p


parser = build_parser()
main_parser = build_main_parser()

# preprocess.py:30-31 builds one FaceAlignment per GPU at import time; here a detector is built on first use, per device index
fa = {}


def get_detector(gpu_id, args, state_dict=None):
    """the FaceAlignment of cuda:<gpu_id> at `args.face_det_precision` and `args.face_det_scale` (its rects are full-frame
    coordinates at any scale, so the crops are cut from the full-resolution frame); `state_dict` (S3FD weights) replaces the
    default face_detection/s3fd.pth when the detector is first built"""
    from . import face_detection
    from .inference import CLI_PRECISION, _det_scale_kw
    precision = CLI_PRECISION[getattr(args, "face_det_precision", "fp32")]
    det_scale = getattr(args, "face_det_scale", 1)
    key = (gpu_id, precision) if det_scale == 1 else (gpu_id, precision, det_scale)
    if key not in fa or state_dict is not None:
        fa[key] = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False,
                                               device='cuda:{}'.format(gpu_id), state_dict=state_dict, precision=precision,
                                               **_det_scale_kw(det_scale))
    return fa[key]


def _out_dir(vfile, args):
    vidname = os.path.basename(vfile).split('.')[0]
    dirname = vfile.split('/')[-2]
    return path.join(args.preprocessed_root, dirname, vidname)


def _read(vfile):
    if not vfile.lower().endswith('.avi'):
        raise ValueError("%s: only uncompressed AVI clips (24-bit BGR video, PCM16 audio) can be decoded here; convert the clip "
                         "(the reference decodes .mp4 with cv2 / ffmpeg, which this package does not use)" % vfile)
    return container.read_avi(vfile)


def _write_jpeg(dst, crop_bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(crop_bgr[:, :, ::-1])).save(dst, format="JPEG", quality=JPEG_QUALITY,
                                                                      subsampling=JPEG_SUBSAMPLING)


_pool = None


def _jpeg_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(JPEG_WORKERS)
    return _pool


_encoder = None


def _crop_encoder(bs):
    """`--jpeg device`: the process's jpeg.CropEncoder (one worker thread and one stream, whatever the number of clips); its file
    writes go to the pool above, bounded as the host path bounds its pending crops"""
    global _encoder
    if _encoder is None:
        from . import jpeg
        _encoder = jpeg.CropEncoder(JPEG_QUALITY, pool=_jpeg_pool())
    _encoder.max_files = 4 * bs
    return _encoder


def process_video_file(vfile, args, gpu_id):
    """preprocess.py:35-66: detect every frame of `vfile` in batches of args.batch_size on cuda:<gpu_id> and write the face crops
    fb[y1:y2, x1:x2] as <i>.jpg.  Returns when every crop is on disk."""
    frames = _read(vfile)["frames"]

    fulldir = _out_dir(vfile, args)
    os.makedirs(fulldir, exist_ok=True)

    det = get_detector(gpu_id, args)
    bs = args.batch_size
    pending = []
    enc = None
    if getattr(args, "jpeg", "host") == "device":
        import torch
        enc = _crop_encoder(bs)
        dev = torch.device('cuda:{}'.format(gpu_id))
    try:
        i = -1
        for lo in range(0, len(frames), bs):
            fb = frames[lo:lo + bs]
            if len(fb) < bs:
                # the ragged last batch runs the full batch's graph (no rebuild per clip); the copies' rects are dropped
                fb = np.concatenate([fb, np.repeat(fb[-1:], bs - len(fb), axis=0)])
            if enc is not None:
                fb = torch.from_numpy(np.ascontiguousarray(fb)).to(dev)        # the batch's one upload: detector and encoder read it
            preds = det.get_detections_for_batch(fb)[:min(bs, len(frames) - lo)]

            boxes, rows, paths = [], [], []
            for j, f in enumerate(preds):
                i += 1
                if f is None:
                    continue

                x1, y1, x2, y2 = f
                if enc is not None:
                    # what the slice fb[j][y1:y2, x1:x2] keeps: numpy cuts a rect that overhangs the frame at its edge
                    box = (min(x1, fb.shape[2]), min(y1, fb.shape[1]), min(x2, fb.shape[2]), min(y2, fb.shape[1]))
                    if box[2] <= box[0] or box[3] <= box[1]:
                        raise ValueError("%s: frame %d: empty face crop %r (cv2.imwrite refuses an empty image)" % (vfile, i, f))
                    boxes.append(box)
                    rows.append(j)
                    paths.append(path.join(fulldir, '{}.jpg'.format(i)))
                    continue
                crop = fb[j][y1:y2, x1:x2]
                if crop.size == 0:
                    raise ValueError("%s: frame %d: empty face crop %r (cv2.imwrite refuses an empty image)" % (vfile, i, f))
                pending.append(_jpeg_pool().submit(_write_jpeg, path.join(fulldir, '{}.jpg'.format(i)), crop))
            if boxes:
                with torch.cuda.device(dev):
                    enc.submit(fb, boxes, paths, frame_index=rows)      # bounded: CropEncoder holds at most two batches back
            while len(pending) > 4 * bs:          # bounded: at most a few batches of crops wait for the encoder
                pending.pop(0).result()
        for p in pending:
            p.result()
        if enc is not None:
            enc.finish()
    finally:
        wait(pending)
        if enc is not None:
            enc.drain()


def process_audio_file(vfile, args):
    """preprocess.py:68-78 (`ffmpeg -i <vfile> -strict -2 <dir>/audio.wav`): the clip's PCM16 track at its own rate and channel
    count as <dir>/audio.wav.  A clip without an audio track gets no audio.wav."""
    a = _read(vfile)
    if a["audio"] is None:
        print("{}: no audio track, no audio.wav".format(vfile))
        return

    fulldir = _out_dir(vfile, args)
    os.makedirs(fulldir, exist_ok=True)

    wavpath = path.join(fulldir, 'audio.wav')
    pcm = np.ascontiguousarray(a["audio"], dtype='<i2')
    with wave.open(wavpath, 'wb') as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(a["audio_sr"]))
        w.writeframes(pcm.tobytes())


def mp_handler(job):
    vfile, args, gpu_id = job
    try:
        process_video_file(vfile, args, gpu_id)
    except KeyboardInterrupt:
        raise
    except Exception:
        traceback.print_exc()


def check_world(ngpu, world):
    """`--ngpu` is 1 (whatever the launch) or the number of processes torch.distributed.run started"""
    if ngpu != 1 and ngpu != world:
        raise ValueError("--ngpu {} but {} process(es) are running: one process drives one GPU, launch with "
                         "`python -m torch.distributed.run --nproc-per-node {} -m wav2lip_amd.preprocess --ngpu {} ...` "
                         "(or pass --ngpu 1)".format(ngpu, world, ngpu, ngpu))


def list_videos(data_root):
    """preprocess.py:85 `glob(data_root/*/*.mp4)`, plus the AVI clips this package can decode; sorted, so that every rank deals the
    same list"""
    return sorted(glob(path.join(data_root, '*/*.mp4')) + glob(path.join(data_root, '*/*.avi')))


def main(args, state_dict=None, backend="nccl"):
    """preprocess.py:80-102.  `args` as `main_parser.parse_args()` (or `parser.parse_args()`) returns it; `state_dict` (S3FD weights) replaces
    face_detection/s3fd.pth; `backend` is the process group's (the tests run two ranks on one device over "gloo")."""
    from . import sharding
    check_world(args.ngpu, int(os.environ.get("WORLD_SIZE", "1")))
    ranks = sharding.init_from_env(backend)
    say = print if ranks.writer else (lambda *a, **k: None)
    try:
        say('Started processing for {} with {} GPUs'.format(args.data_root, ranks.world))

        filelist = list_videos(args.data_root)
        mine = [vfile for i, vfile in enumerate(filelist) if i % ranks.world == ranks.rank]
        gpu_id = ranks.device.index if ranks.device.index is not None else 0
        get_detector(gpu_id, args, state_dict)

        for vfile in mine:
            mp_handler((vfile, args, gpu_id))

        say('Dumping audios...')

        for vfile in mine:
            try:
                process_audio_file(vfile, args)
            except KeyboardInterrupt:
                raise
            except Exception:
                traceback.print_exc()
                continue
        if ranks.dist is not None and ranks.world > 1:
            ranks.dist.barrier()
    finally:
        ranks.close()


if __name__ == '__main__':
    main(main_parser.parse_args())
