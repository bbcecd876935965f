"""mqr -- MI355X-native TSDF fusion path for Quest depth captures."""
__version__ = "0.1.0"

from . import compare_mesh_to_ground_truth  # noqa: E402,F401  (loads no library: the HIP library opens on first call)
from .downsample_mesh import downsample_mesh  # noqa: E402,F401  (the function; its module: ``from mqr.downsample_mesh import ...``)
from .geometry import simplify_vertex_clustering  # noqa: E402,F401
