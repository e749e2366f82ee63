from .triangulation import LandmarksTriangulator  # noqa: F401
from .window_ba import WindowBundleAdjuster, pack_windows, solve_windows  # noqa: F401
from .window_structure import WindowStructureRefiner, refine_windows  # noqa: F401
from .structure_loop import StructureLoop, ring_full, ring_slots  # noqa: F401
