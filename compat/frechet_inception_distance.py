"""Shim so that the reference's `from frechet_inception_distance import frechet_inception_distance` (model_wrapper.py:16) resolves
to the MI355X implementation."""
from semantic_pyramid_for_image_generation_amd.fid import frechet_inception_distance  # noqa: F401
