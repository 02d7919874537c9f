"""TSDF fusion of rendered views into a block-sparse volume on the GPU, and point-cloud / mesh extraction: what the
toolkit's `ExportTSDF` / `ExportPointCloud` commands do with Open3D on the CPU (gs_toolkit/scripts/exporter.py:151-308,
exporter/tsdf_fusion.py).  HIP kernels behind the C ABI (`gsr_tsdf_*`, include/gsraster.h; csrc/tsdf.hip); torch for
memory and streams only; no CPU fallback.  DESIGN.md section 4.5.  `clean_mesh` / `mesh_components` (`gsr_mesh_*`,
csrc/mesh_clean.hip) are the exporter's cleaning step without pymeshlab: DESIGN.md section 4.6.  `MeshDistance` /
`surface_distance` (`gsr_mesh_bvh_build`, `gsr_mesh_distance_*`, csrc/mesh_distance.hip) measure the result against a
ground-truth mesh as gs_toolkit/evaluation/surface_distance does: DESIGN.md section 4.7."""
from .volume import TSDFVolume, invert_viewmat  # noqa: F401
from .fuse import export_mask, fuse_views, read_poses_json, view_depth  # noqa: F401
from .mesh import clean_mesh, mesh_components  # noqa: F401
from .distance import MeshDistance, distance_stats, surface_distance  # noqa: F401
