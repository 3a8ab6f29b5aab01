from .dataset import TargetEncoder, build_target_luts  # noqa: F401
from .loader import DeviceAugmentLoader, PngPairDataset, RaggedBatch, ragged_collate  # noqa: F401
from .augment import DeviceAugment  # noqa: F401
from .decode import DeviceDecode, HedgedLabels, RaggedLabels, WindowPlan, plan_windows, window_profile  # noqa: F401
from .score import DeviceScore, SourceScores, build_score_tables  # noqa: F401
from .postprocess import ComponentTables, DevicePostprocess, build_component_tables  # noqa: F401
from .boundary import BoundaryScores, DeviceBoundaryScore  # noqa: F401
from .instances import DeviceInstanceScore, InstanceScores  # noqa: F401
from .calibration import CalibrationScores, DeviceCalibrationScore  # noqa: F401
from .hedge import Hedge  # noqa: F401
from .mix import DeviceMix  # noqa: F401
from .consensus import ConsensusLabels, DeviceConsensus  # noqa: F401
