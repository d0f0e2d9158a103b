from .function import rasterize, rasterize_with_tiles, RasterOut
from .wide import rasterize_wide, render_features
from ..data_types import RasterConfig

__all__ = ['rasterize', 'rasterize_with_tiles', 'rasterize_wide', 'render_features', 'RasterConfig', 'RasterOut']
