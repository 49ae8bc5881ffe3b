"""`face_detection` with the reference's surface (face_detection/__init__.py, api.py): `FaceAlignment`, `LandmarksType`,
`NetworkSize`; the S3FD detector behind it runs on the HIP path (wav2lip_amd/face_detection/s3fd.py).  `detect_many` /
`DetectJob` (wav2lip_amd/face_detection/many.py) run `inference.face_detect` for many clips in shared detector batches; `FaceTrack`
(wav2lip_amd/face_detection/track.py) is the value their opt-in `face_track=` takes, `SceneCuts`
(wav2lip_amd/face_detection/scene.py) the value of their opt-in `scene_cuts=`, `TrackSpans`
(wav2lip_amd/face_detection/spans.py) the value of `detect_many`'s opt-in `track_spans=`, `AllFaces`
(wav2lip_amd/face_detection/faces.py) the value of its opt-in `all_faces=`."""
from .api import FaceAlignment, LandmarksType, NetworkSize  # noqa: F401
from .faces import AllFaces  # noqa: F401
from .many import DetectJob, detect_many  # noqa: F401
from .s3fd import s3fd  # noqa: F401
from .scene import SceneCuts  # noqa: F401
from .spans import TrackSpans  # noqa: F401
from .track import FaceTrack  # noqa: F401
