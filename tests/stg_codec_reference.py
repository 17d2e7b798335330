"""The decode of the reference's ``STGPngCompression.decompress`` (gsplat/compression/stg_compression.py:124-143, 196-223, 271-304,
350-378, 429-461) restated in numpy, from planes and meta.json entries: what the GPU tests of the spacetime codec compare against.
tests/test_stg_codec_cpu.py pins it bit for bit to the tensors the reference itself returned (tests/golden/stg_codec.npz).

The reference divides the integer image by ``2^bits - 1`` in numpy (float64), multiplies by the float32 ``maxs - mins``, adds the
float32 ``mins`` (both promoted to float64 by torch) and casts to the meta's dtype; the means then go through
``sign(y) * expm1(|y|)`` in float32 (torch's expm1, so that the last bit is the reference's)."""
import numpy as np
import torch

FILES = {"means": ("means_l.png", "means_u.png"), "motion": ("motion_0.png", "motion_1.png", "motion_2.png")}


def files_of(name):
    return FILES.get(name, (f"{name}.png",))


def decode_attribute(name, planes, m):
    """planes: the uint8 images of ``files_of(name)`` in that order; m: the meta.json entry."""
    planes = [np.asarray(p) for p in planes]
    if name == "means":
        img, levels = (planes[1].astype(np.uint16) << 8) + planes[0], 2**16 - 1
    elif name == "motion":
        img, levels = np.concatenate(planes, axis=-1), 2**8 - 1
    else:
        bits = int(m.get("quantization", 8))
        img, levels = planes[0] >> (8 - bits), 2**bits - 1
    mins, maxs = np.asarray(m["mins"], np.float32), np.asarray(m["maxs"], np.float32)
    grid = (img / levels).reshape(-1, mins.size) * (maxs - mins).astype(np.float64) + mins.astype(np.float64)
    out = grid.reshape(m["shape"]).astype(m["dtype"])
    if name == "means":
        y = torch.from_numpy(out)
        out = (torch.sign(y) * torch.expm1(torch.abs(y))).numpy()
    return out
