from .correlation import CorrelationScores, DeviceCorrelation  # noqa: F401
from .privacy import DevicePrivacy, PrivacyGuard, PrivacyScores  # noqa: F401
from .fed_privacy import ShardedGuard, ShardedPrivacy, ShardedScores, ShardPrivacy, merge_partials  # noqa: F401
from .fidelity import DeviceFidelity, FidelityScores  # noqa: F401
from .utility_device import DeviceUtility, UtilityScores  # noqa: F401
from .forest_device import DeviceForest, ForestScores  # noqa: F401
from .mlp_device import DeviceMLP, MLPScores  # noqa: F401
