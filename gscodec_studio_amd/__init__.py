"""gscodec_studio_amd -- MI355X-native rasterize + quantize hot path of GSCodec Studio.

Public surface (mirrors the reference's ``gsplat`` package for this path only):
  rendering.rasterization, the operator functions of ``_wrapper`` and
  ``compression_simulation.{CompressionSimulation, STGCompressionSimulation, fake_quantize_ste, STE}`` and
  ``optimizers.{Adam, SelectiveAdam, step_all, visibility_mask}`` and ``losses.{fused_ssim, photometric_loss}`` and
  ``strategy.{Strategy, DefaultStrategy, MCMCStrategy, STG_Strategy, Modified_STG_Strategy}`` (``from gscodec_studio_amd.strategy import ...``, as in the reference) with
  ``relocation.compute_relocation``, and ``bilagrid.{BilateralGrid, slice, slice_image, total_variation_loss,
  color_affine_transform}`` (``from gscodec_studio_amd.bilagrid import ...`` in place of ``from lib_bilagrid import ...``) with the
  evaluation's ``color_correct.color_correct`` (``from gscodec_studio_amd.color_correct import color_correct``), and the 2D Gaussian splatting
  renderer ``rasterization_2dgs`` with its operators ``fully_fused_projection_2dgs`` / ``rasterize_to_pixels_2dgs`` (``surfel.py``) and
  ``utils.{depth_to_points, depth_to_normal}``, and the spacetime trainer's colour decoder
  ``dynamic.{Sandwich, getcolormodel, decode_colors, trbfunction}`` (``from gscodec_studio_amd.dynamic import getcolormodel, trbfunction``
  in place of ``from helper.STG.helper_model import ...``; ``dynamic.render_dynamic(..., decoder=, rays=)`` applies it after the render),
  and the static trainer's appearance module ``appearance.AppearanceOptModule`` (``from gscodec_studio_amd.appearance import
  AppearanceOptModule`` in place of ``from utils import AppearanceOptModule``; ``module.colors(...)`` is the fused form of its call site),
  and the trainers' neighbour search ``utils.{knn, knn_search, init_scales}`` (``knn.py``: ``from gscodec_studio_amd.utils import knn``
  in place of ``from utils import knn``; exact grid k-NN on the GPU, ``init_scales`` is the three lines that size the initial splats),
  and ``.ply`` files in the INRIA 3DGS layout without plyfile: ``utils.{load_ply, save_ply, load_ply_to_rasterizer_inputs,
  read_ply_header}`` (``ply.py``, ``csrc/ply.hip``), with ``utils.{rgb_to_sh, set_random_seed}`` beside them, so that
  ``from utils import knn, rgb_to_sh, set_random_seed, load_ply`` reads ``from gscodec_studio_amd.utils import ...``,
  and the file codecs of ``compression`` (``PngCompression``, ``EntropyCodingCompression``, ``HevcCompression``,
  ``STGPngCompression`` and, for a sequence of splat dictionaries such as one ``.ply`` per frame, ``SeqHevcCompression``:
  ``from gscodec_studio_amd.compression import SeqHevcCompression`` in place of ``from gsplat.compression.seq_hevc_compression import ...``).
"""
from ._wrapper import (
    accumulate,
    fully_fused_projection,
    isect_offset_encode,
    isect_tiles,
    persp_proj,
    proj,
    quat_scale_to_covar_preci,
    rasterize_to_indices_in_range,
    rasterize_to_pixels,
    selective_adam_update,
    spherical_harmonics,
    spherical_harmonics_shared,
    world_to_cam,
)
from .rendering import rasterization, rasterization_2dgs
from .surfel import fully_fused_projection_2dgs, rasterize_to_pixels_2dgs
from . import utils
from .appearance import AppearanceOptModule
from .version import __version__


def __getattr__(name):  # (lazy: the codec module is not on the training path)
    if name == "PngCompression":  # reference: gsplat/__init__.py:3
        from .compression import PngCompression

        return PngCompression
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = [
    "rasterization", "fully_fused_projection", "spherical_harmonics", "spherical_harmonics_shared",
    "isect_tiles", "isect_offset_encode", "rasterize_to_pixels", "quat_scale_to_covar_preci", "proj", "persp_proj",
    "world_to_cam", "rasterize_to_indices_in_range", "accumulate", "selective_adam_update", "PngCompression", "__version__",
    "rasterization_2dgs", "fully_fused_projection_2dgs", "rasterize_to_pixels_2dgs", "utils",
    "AppearanceOptModule",
]
