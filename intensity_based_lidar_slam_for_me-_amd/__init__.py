"""lislam: MI355X-native intensity-LiDAR SLAM front-end hot path.

Import with ``importlib.import_module("intensity_based_lidar_slam_for_me-_amd")`` (the directory
name is not a Python identifier).  The compute path is the HIP library ``liblislam.so`` built by
``__graft_entry__.build()``; there is no CPU fallback.
"""
from . import backend, bow, intensity, keyframes, loop, mapping, native, place, posegraph, synth  # noqa: F401
from .bow import BowDatabase, BowTrainer, Vocabulary  # noqa: F401
from .backend import LoopBackend  # noqa: F401
from .keyframes import KeyframePool, KeyframeSelector, close_loops  # noqa: F401
from .place import ScanContext  # noqa: F401
from .posegraph import PoseGraph  # noqa: F401
from .frontend import Batch, Context, Features, ImageHandler, LaserOdometry, ScanRegistration, eval_factors  # noqa: F401

__all__ = ["backend", "bow", "intensity", "keyframes", "loop", "mapping", "native", "place", "posegraph", "synth", "Batch", "BowDatabase", "BowTrainer", "Context", "Features", "ImageHandler", "KeyframePool", "KeyframeSelector", "LaserOdometry", "LoopBackend",
           "PoseGraph", "ScanContext", "ScanRegistration", "Vocabulary", "close_loops", "eval_factors"]
