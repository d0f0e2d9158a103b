from .knn import knn, mean_knn_dist2
from .coverage import camera_coverage, pack_cameras, Coverage

__all__ = ["knn", "mean_knn_dist2", "camera_coverage", "pack_cameras", "Coverage"]
