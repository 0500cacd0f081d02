"""icpslam_amd -- MI355X (gfx950) ICP scan-matching core behind icpslam's ICP-odometry call.

Only what the hot path needs: csrc/ (HIP kernels + C-ABI, built into libicpgpu.so), the ctypes binding,
the PCL-Registration-shaped host mirror and the synthetic scan generator.  No CPU fallback.
"""
from ._lib import GICP, GICP_INNER_EXACT, NDT, NDT_LINE_SEARCH_MORE_THUENTE, NDT_LINE_SEARCH_PCL18, P2PLANE, GICP_INNER_QUADRATIC, NN_AUTO, NN_BRUTE, NN_GRID, P2P_SVD, STATE_NAMES, IcpGpuError, Params, Profile, Result  # noqa: F401
from .registration import CorrespondenceRejectorMedianDistance, CorrespondenceRejectorOneToOne, CorrespondenceRejectorTrimmed  # noqa: F401
from .registration import CorrespondenceRejectorSurfaceNormal, solve_symmetric_point_to_plane  # noqa: F401
from .registration import CorrespondenceRejectorSampleConsensus  # noqa: F401
from ._lib import REJECT_MEDIAN_DISTANCE, REJECT_ONE_TO_ONE, REJECT_SURFACE_NORMAL, REJECT_TRIMMED, Rejector  # noqa: F401
from .registration import RadiusOutlierRemoval, StatisticalOutlierRemoval  # noqa: F401
from .registration import CropBox, FarthestPointSampling, PassThrough, UniformSampling, crop_box_matrix, seeded_first_row  # noqa: F401
from .registration import KdTree, KdTreeFLANN  # noqa: F401
from .registration import NormalEstimation  # noqa: F401
from .registration import FPFH_BINS, FPFHEstimation  # noqa: F401
from .registration import FeatureKdTree, SampleConsensusPrerejective  # noqa: F401
from .registration import EuclideanClusterExtraction, RegionGrowing  # noqa: F401
from .registration import SEGMENT_RECORD, MomentOfInertiaEstimation  # noqa: F401
from .registration import ExtractIndices, SACSegmentation, SACSegmentationFromNormals  # noqa: F401
from .registration import ISSKeypoint3D  # noqa: F401
from .registration import BoundaryEstimation, ISSKeypoint3DBorder  # noqa: F401
from ._lib import SAC_RANSAC, SACMODEL_PERPENDICULAR_PLANE, SACMODEL_PLANE  # noqa: F401
from ._lib import SACMODEL_CYLINDER, SACMODEL_NORMAL_PLANE  # noqa: F401
from .registration import ProgressiveMorphologicalFilter  # noqa: F401
from ._lib import MORPH_CLOSE, MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, PMF_MAX_PASSES  # noqa: F401
from .registration import Context, GeneralizedIterativeClosestPoint, IterativeClosestPoint, IterativeClosestPointWithNormals, NormalDistributionsTransform  # noqa: F401

__all__ = ["Context", "IterativeClosestPoint", "GeneralizedIterativeClosestPoint", "IterativeClosestPointWithNormals", "NormalDistributionsTransform", "StatisticalOutlierRemoval", "RadiusOutlierRemoval", "PassThrough", "CropBox", "UniformSampling", "FarthestPointSampling", "crop_box_matrix", "seeded_first_row", "KdTree", "KdTreeFLANN", "NormalEstimation", "FPFHEstimation", "FPFH_BINS", "FeatureKdTree", "SampleConsensusPrerejective", "EuclideanClusterExtraction", "RegionGrowing", "MomentOfInertiaEstimation", "SEGMENT_RECORD", "ISSKeypoint3D", "ISSKeypoint3DBorder", "BoundaryEstimation", "SACSegmentation", "SACSegmentationFromNormals", "ExtractIndices", "SACMODEL_CYLINDER", "SACMODEL_NORMAL_PLANE", "SACMODEL_PLANE", "SACMODEL_PERPENDICULAR_PLANE", "SAC_RANSAC", "ProgressiveMorphologicalFilter", "MORPH_ERODE", "MORPH_DILATE", "MORPH_OPEN", "MORPH_CLOSE", "PMF_MAX_PASSES", "IcpGpuError", "Params", "Result",
           "Profile", "P2P_SVD", "GICP", "P2PLANE", "NDT", "NDT_LINE_SEARCH_PCL18", "NDT_LINE_SEARCH_MORE_THUENTE", "GICP_INNER_EXACT", "GICP_INNER_QUADRATIC",
           "NN_AUTO", "NN_BRUTE", "NN_GRID", "STATE_NAMES"]
