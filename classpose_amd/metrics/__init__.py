"""Panoptic-quality evaluation on the device: the interface of the reference's ``classpose.metrics``."""
from .pq import compute_binary_pq_metrics, compute_multiclass_pq_metrics
from .utils import check_and_coherce_if_necessary, load_masks

__all__ = ["compute_binary_pq_metrics", "compute_multiclass_pq_metrics", "check_and_coherce_if_necessary", "load_masks"]
