"""Train-time compression simulation: per-splat quantize/dequantize STE hooks.

Counterpart of the quantizer part of the reference's ``gsplat/compression_simulation``
(ops.py + the quantization hooks of simulation.py) and of its factorized-prior bits estimator
(entropy_model.py) and of the learnable shN mask (ada_mask.py), and of its hash-grid Gaussian
entropy model (gaussian_distribution_model.py, ``Entropy_gaussian``), which ``HashGridCompressionSimulation`` wires up.
"""
from .ada_mask import AnnealingMask
from .entropy_model import Entropy_factorized_optimized_refactor, Entropy_gaussian, LowerBound
from .gaussian_distribution_model import GridEncoder, STE_binary, STE_multistep, hash_based_estimator, mix_3D2D_encoding
from .ops import STE, fake_quantize_ste
from .simulation import CompressionSimulation, HashGridCompressionSimulation, STGCompressionSimulation

__all__ = ["AnnealingMask", "STE", "fake_quantize_ste", "CompressionSimulation", "STGCompressionSimulation",
           "HashGridCompressionSimulation", "Entropy_factorized_optimized_refactor", "Entropy_gaussian", "LowerBound",
           "GridEncoder", "STE_binary", "STE_multistep", "hash_based_estimator", "mix_3D2D_encoding"]
