from .knn import knn, mean_knn_dist2

__all__ = ["knn", "mean_knn_dist2"]
