from .knn import knn, mean_knn_dist2, knn_query
from .coverage import camera_coverage, pack_cameras, Coverage
from .relocate import relocate_gaussians3d, perturb_positions

__all__ = ["knn", "mean_knn_dist2", "knn_query", "camera_coverage", "pack_cameras", "Coverage", "relocate_gaussians3d",
           "perturb_positions"]
