from ._lib import load, OrbHipError, KP_DTYPE  # noqa: F401
from .extractor import ORBextractor, stereo_matches  # noqa: F401
from .matcher import ORBmatcher, QUERY_DTYPE  # noqa: F401
from .lba import LbaWindows, synth_window  # noqa: F401
from .frame import FrameOps, Camera  # noqa: F401
from .keyframe_db import KeyFrameDatabase  # noqa: F401
from .sim3 import Sim3Solver  # noqa: F401
from .two_view import TwoViewReconstruction  # noqa: F401
from .covisibility import CovisibilityGraph  # noqa: F401
from .new_keyframe import NewKeyFrame  # noqa: F401
from .local_ba import LocalBA  # noqa: F401

__all__ = ["load", "OrbHipError", "KP_DTYPE", "ORBextractor", "stereo_matches", "ORBmatcher", "QUERY_DTYPE", "LbaWindows", "synth_window", "FrameOps", "Camera", "KeyFrameDatabase", "Sim3Solver", "TwoViewReconstruction", "CovisibilityGraph", "NewKeyFrame", "LocalBA"]
