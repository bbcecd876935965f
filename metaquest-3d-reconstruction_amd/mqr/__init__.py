"""mqr -- MI355X-native TSDF fusion path for Quest depth captures."""
__version__ = "0.1.0"

from . import compare_mesh_to_ground_truth  # noqa: E402,F401  (loads no library: the HIP library opens on first call)
