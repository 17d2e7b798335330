"""Densification strategies (counterpart of the reference's ``gsplat.strategy``): ``DefaultStrategy`` (the 3DGS paper's clone /
split / prune / opacity reset), ``MCMCStrategy`` (relocation, growth up to a cap, position noise) and the spacetime trainer's
``STG_Strategy`` / ``Modified_STG_Strategy`` (growth for a number of refinements, then pruning; an omega / rotation freeze late in
training), with the reference's fields, defaults and schedule.  Their per-step work is one HIP launch each (``ops.densify_stats``,
``ops.inject_noise_to_position``, ``ops.stg_freeze_grads``).

    from gscodec_studio_amd.strategy import DefaultStrategy, MCMCStrategy, STG_Strategy, Modified_STG_Strategy
"""
from .base import Strategy
from .default import DefaultStrategy
from .mcmc import MCMCStrategy
from .stg import Modified_STG_Strategy, STG_Strategy

# (the star-import surface stays the static trainers' three names, as tests/test_strategy_cpu.py pins it; the spacetime strategies
# are imported by name, as the dynamic trainer does)
__all__ = ["Strategy", "DefaultStrategy", "MCMCStrategy"]
