"""Hot-path subset of manifold_gp.utils (manifold_gp/utils/__init__.py:3-18): NearestNeighbors,
bump_function, the training loops `manifold_informed_train` (precision form) / `vanilla_train` / `laplace_train` (the
Laplace evidence of the node fits, beyond the reference) and the metrics caller `test_model`.  Dataset loaders and plotting are out of scope."""
from .nearest_neighbors import NearestNeighbors
from .torch_utils import bump_function
from .test_model import test_model
from .train_model import laplace_train, manifold_informed_train, vanilla_train

__all__ = ["NearestNeighbors", "bump_function", "manifold_informed_train", "vanilla_train", "test_model", "laplace_train"]
