"""gims_amd -- the GIMS matcher hot path (models/gmatcher.py + models/agc.py of songxf1024/GIMS) on MI355X.

Public surface mirrors the reference: ``GMatcher(config).forward(data)`` and ``Matching(config).forward(data)``.
Kernels live in ``gims_amd/csrc`` (HIP, gfx950) behind the C ABI of ``include/gims_hip.h``.
"""
from .gmatcher import GMatcher, ImageFeatures  # noqa: F401
from .matching import Matching  # noqa: F401
from .baselines import mnn, nn_match_pairs, nndr  # noqa: F401
from .augment import ColorAug, ColorAugPlan  # noqa: F401
from .verify import (epipolar_error, estimate_pose, find_fundamental, find_homography, pose_error, pose_summary,  # noqa: F401
                     verify_pairs)
from .tracks import Tracks, build_tracks  # noqa: F401
from .triangulate import Points3D, cameras_from_pose, triangulate_tracks  # noqa: F401
from .resect import Poses, absolute_pose, resect_images  # noqa: F401
from .bundle import Adjusted, bundle_adjust  # noqa: F401
from .pairs import PairSelection, select_pairs  # noqa: F401
from .guided import guided_match_features, guided_match_pairs  # noqa: F401

__all__ = ["GMatcher", "ImageFeatures", "Matching", "nndr", "mnn", "nn_match_pairs", "ColorAug", "ColorAugPlan", "find_homography", "find_fundamental", "verify_pairs",
           "estimate_pose", "pose_error", "epipolar_error", "pose_summary", "build_tracks", "Tracks",
           "triangulate_tracks", "Points3D", "cameras_from_pose", "resect_images", "Poses", "absolute_pose", "bundle_adjust", "Adjusted",
           "select_pairs", "PairSelection", "guided_match_pairs", "guided_match_features"]
