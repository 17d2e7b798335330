"""On-disk quantized attribute format.

* ``grid_codec``: the min-max grid quantizer behind the reference's ``PngCompression``
  (gsplat/compression/png_compression.py) -- 8-bit, k-bit and 16-bit planes and their exact inverse -- as HIP kernels, plus
  the attribute-level pre/post-processing (log transform of the means, quaternion normalisation, square crop);
* ``decode``: the compressed planes decoded STRAIGHT INTO ``rasterization()``'s inputs by one kernel
  (``decode_to_rasterizer_inputs``), the K-means codebook of the higher SH bands (``kmeans_decode`` bit-exact against the
  reference's ``_decompress_kmeans``; ``kmeans_encode`` = seeded Lloyd iteration writing the same format), and the splat
  ordering in front of the grid codec (``sort_splats`` = PLAS, an external package as in the reference; ``morton_order`` =
  deterministic substitute on the means alone).
* ``grid_sort``: ``grid_sort_order`` / ``sort_splats_grid``, the ordering over EVERY attribute that PLAS stands for, as the
  library's own integer algorithm on the GPU (csrc/grid_sort.hip: box blur, random groups through the radix sort, best-of-24
  assignment), defined by the numpy code ``grid_sort_reference`` that the kernels match element for element;
  ``use_sort="grid"`` of the two codecs below.
* ``kmeans``: ``kmeans_fit`` / ``KMeans``, the clustering behind the shN codebook that the reference takes from ``torchpq``
  (manhattan distance), in 24-bit fixed point on the GPU (csrc/kmeans.hip: one v_sad_u32 per element of the assignment, integer
  atomics in the update), defined by the numpy code ``kmeans_reference`` that the kernels match element for element;
  ``kmeans_encode(method="fixed")`` and ``kmeans_method="fixed"`` of the two codecs below.

* ``_container``: the directory layer under the three file codecs below -- the preparation of the splats (opacity filter, log
  transform, normalised quats, square crop, ``use_sort`` ordering), the loop over the attributes with ``meta.json``, the
  empty-attribute rule and the ``<name>.npz`` fallback, the PNG plane files and their names, a self-contained 8-bit PNG reader /
  writer (``png_read`` / ``png_write``; the image has no imageio) and the masked K-means file pair.  Each codec hands it one
  callback per direction that says what to do with an attribute.

* ``png_compression``: the file level -- ``PngCompression.compress(dir, splats)`` / ``decompress(dir)`` with the reference's
  directory layout (PNG image grids, ``shN.npz`` + ``mask.bin``, ``meta.json``), so directories written by either
  implementation are read by the other.

* ``stg_compression``: ``STGPngCompression``, the reference's ``--compression stg`` of the two dynamic trainers -- the spacetime
  attributes (means, scales, quats, opacities, trbf_center, trbf_scale, motion in three images, omega, colors, features_dir,
  features_time) as PNG image grids in the reference's layout; ``decompress`` decodes all of them with ONE launch
  (``decode_to_dynamic_inputs``, csrc/codec.hip) into the RAW parameter dict ``dynamic.render_dynamic`` takes.

* ``entropy_coding_compression``: ``EntropyCodingCompression``, the reference's ``--compression entropy_coding`` -- the same
  directory, with the scales and the quats rANS-coded on the GPU by ``ans`` (csrc/ans.hip: histogram, lane-per-stream encode,
  pack, decode).  The reference takes its coder from the ``constriction`` package; the bitstream here is this project's own,
  defined by the numpy coder ``ans_reference`` that the kernels match byte for byte.
* ``gauss_ans``: the hash-grid Gaussian route of the same class (``_compress_gaussian_ans``, chosen through the registry): every
  symbol coded against the Gaussian that the trained ``Entropy_gaussian`` predicts at the splat's position (csrc/gauss_ans.hip:
  the regressor's MLP in one stated float32 order, lane-per-stream encode and decode at 16-bit resolution), with the reference's
  model files and meta keys around a bitstream defined by the numpy coder ``gauss_ans_reference``.

* ``hevc_compression``: ``HevcCompression``, the reference's ``--compression hevc`` -- the same directory, with scales, quats,
  opacities and sh0 as lossy transform-coded planes under HEVC's quantisation parameter ``qp``, the one codec with a rate knob.
  The reference shells out to ffmpeg / libx265; the payload here is this project's own bitstream, not a replication of x265.
* ``plane_codec``: ``plane_encode`` / ``plane_decode``, that payload on the GPU (csrc/plane_codec.hip: HEVC's 8 x 8 integer
  transform and flat quantiser with one lane per block, then the rANS streams over 15 static tables), defined by the numpy code
  ``plane_codec_reference`` that the kernels match byte for byte.

* ``seq_hevc_compression``: ``SeqHevcCompression``, the reference's codec for a SEQUENCE of splat dictionaries (one ``.ply`` per
  frame of a dynamic scene): ``reorganize`` / ``compress`` / ``decompress`` / ``deorganize`` with the reference's fields, every
  attribute a video of grids, frame t predicted from the decoded frame t - 1 (or all-intra).  The reference shells out to
  ffmpeg / libx265 here too; the payload is this project's own bitstream, the means are lossless.
* ``plane_seq_codec``: ``plane_seq_encode`` / ``plane_seq_decode``, that payload on the GPU (the sequence kernels of
  csrc/plane_codec.hip: the plane codec's stages with one lane owning a block through all frames, the reconstruction in registers,
  the closed loop in one launch), defined by the numpy code ``plane_seq_codec_reference`` that the kernels match byte for byte.
"""
from .decode import decode_to_dynamic_inputs, decode_to_rasterizer_inputs, kmeans_decode, kmeans_encode, morton_order, reorder_splats, sort_splats
from ._container import png_read, png_write
from .png_compression import PngCompression
from .ans import ans_decode, ans_encode, normalize_frequencies, symbol_histogram
from .gauss_ans import gauss_ans_decode, gauss_ans_encode, gaussian_params
from .entropy_coding_compression import EntropyCodingCompression
from .stg_compression import STGPngCompression
from .plane_codec import plane_decode, plane_encode
from .hevc_compression import HevcCompression
from .plane_seq_codec import plane_seq_decode, plane_seq_encode
from .seq_hevc_compression import SeqHevcCompression
from .grid_sort import grid_sort_order, sort_splats_grid
from .kmeans import KMeans, kmeans_fit
from .grid_codec import (
    compress_to_arrays,
    decompress_from_arrays,
    dequantize_grid,
    inverse_log_transform,
    log_transform,
    quantize_grid,
    quantize_grid_sequence,
)

__all__ = ["quantize_grid", "quantize_grid_sequence", "dequantize_grid", "compress_to_arrays", "decompress_from_arrays", "log_transform",
           "inverse_log_transform", "decode_to_rasterizer_inputs", "kmeans_decode", "kmeans_encode", "morton_order",
           "sort_splats", "reorder_splats", "PngCompression", "png_read", "png_write", "EntropyCodingCompression", "ans_encode",
           "ans_decode", "normalize_frequencies", "symbol_histogram", "grid_sort_order", "sort_splats_grid", "STGPngCompression",
           "decode_to_dynamic_inputs", "KMeans", "kmeans_fit", "gaussian_params", "gauss_ans_encode", "gauss_ans_decode",
           "HevcCompression", "plane_encode", "plane_decode", "SeqHevcCompression", "plane_seq_encode", "plane_seq_decode"]
