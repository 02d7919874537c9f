"""On-disk formats either side of the rasterizer."""
from .ply import read_gaussian_ply, write_gaussian_ply  # noqa: F401
from .ply import read_mesh_ply, read_point_cloud_ply, write_mesh_ply, write_point_cloud_ply  # noqa: F401
from .stl import read_stl  # noqa: F401
from .compressed import compress_gaussians, decompress_gaussians, read_compressed, write_compressed  # noqa: F401
