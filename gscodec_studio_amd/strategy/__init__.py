"""Densification strategies (counterpart of the reference's ``gsplat.strategy``): ``DefaultStrategy`` (the 3DGS paper's clone /
split / prune / opacity reset) and ``MCMCStrategy`` (relocation, growth up to a cap, position noise), with the reference's fields,
defaults and schedule.  Their per-step work is one HIP launch each (``ops.densify_stats``, ``ops.inject_noise_to_position``).

    from gscodec_studio_amd.strategy import DefaultStrategy, MCMCStrategy
"""
from .base import Strategy
from .default import DefaultStrategy
from .mcmc import MCMCStrategy

__all__ = ["Strategy", "DefaultStrategy", "MCMCStrategy"]
