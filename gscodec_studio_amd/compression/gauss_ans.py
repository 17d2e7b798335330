"""The hash-grid Gaussian route of ``EntropyCodingCompression``'s entropy coder on the GPU: 8-bit symbols [N, C], coded against a
Gaussian per splat and channel that the trained ``Entropy_gaussian`` predicts from the splat's position  <->  the ``<name>.bin``
container of ``gauss_ans_reference`` (which defines the format; the kernels of csrc/gauss_ans.hip write the same bytes).

    gaussian_params(entropy_model, positions, mins, maxs)  -> (mu_q int16 [N, C], k uint8 [N, C])
                                                               hash-grid encoder launch + gs_gauss_ans_params (the MLP, the
                                                               normalisation and the quantisation, in one stated float32 order)
    gauss_ans_encode(symbols, mu_q, k, stream_len=1024)    -> container bytes   (transpose, encode, scan, pack)
    gauss_ans_decode(blob, mu_q, k, device)                -> symbols [N, C]    (container validated on the host before any launch)

``mu_q`` and ``k`` are [N, C] views of channel-major [C, N] storage, the layout the coder kernels read; any [N, C] tensor works.
One lane owns one stream of ``stream_len`` symbols of one channel."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from .. import _backend as B
from . import gauss_ans_reference as R
from ._ans_streams import _stream, check_symbols, decode_buffers, encode_streams

MAX_CHANNELS = 8  # of the params kernel: the regressor's weights live in LDS, its accumulators in registers
MAX_CODER_CHANNELS = 16

_DEVICE_TABLES: Dict[torch.device, Tuple[Tensor, Tensor]] = {}


def _tables(dev: torch.device) -> Tuple[Tensor, Tensor]:
    """(G as int16 bit patterns [64, 4073], thresholds float32 [63]) on ``dev``, uploaded once per device."""
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    t = _DEVICE_TABLES.get(dev)
    if t is None:
        g = torch.from_numpy(R.gaussian_table().view(np.int16).copy()).to(dev)
        tau = torch.from_numpy(R.level_thresholds().copy()).to(dev)
        t = _DEVICE_TABLES[dev] = (g, tau)
    return t


def check_entropy_model(entropy_model) -> int:
    """Refuse anything but the reference's ``hash_based_estimator`` shape behind ``entropy_model.param_regressor`` (ValueError)
    and return its channel count: four sign-binarised grids of 2 features with 48 outputs in all, and
    ``Linear(48, 5C)``, ``ReLU``, ``Linear(5C, 2C)``."""
    pr = getattr(entropy_model, "param_regressor", None)
    grid, mlp = getattr(pr, "hash_grid", None), getattr(pr, "mlp_regressor", None)
    encoders = [getattr(grid, f"encoding_{a}", None) for a in ("xyz", "xy", "xz", "yz")]
    if pr is None or grid is None or mlp is None or any(e is None for e in encoders):
        raise ValueError("the Gaussian codec needs an Entropy_gaussian-like module: param_regressor.hash_grid.encoding_{xyz,xy,xz,yz} "
                         "and param_regressor.mlp_regressor")
    c = int(getattr(pr, "channel", 0))
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"the Gaussian codec covers 1..{MAX_CHANNELS} channels per attribute, the entropy model has {c}")
    if any(not e.ste_binary or e.n_features != 2 for e in encoders) or grid.output_dim != R.N_FEATURES:
        raise ValueError(f"the Gaussian codec stores one bit per table entry: it needs four ste_binary grids of 2 features with "
                         f"{R.N_FEATURES} outputs in all, got output_dim = {grid.output_dim}")
    hid = R.HIDDEN_PER_CHANNEL * c
    ok = (isinstance(mlp, nn.Sequential) and len(mlp) == 3 and isinstance(mlp[0], nn.Linear) and isinstance(mlp[1], nn.ReLU)
          and isinstance(mlp[2], nn.Linear) and tuple(mlp[0].weight.shape) == (hid, R.N_FEATURES) and mlp[0].bias is not None
          and tuple(mlp[2].weight.shape) == (2 * c, hid) and mlp[2].bias is not None)
    if not ok:
        raise ValueError(f"the Gaussian codec needs mlp_regressor = Linear({R.N_FEATURES}, {hid}), ReLU, Linear({hid}, {2 * c})")
    return c


@torch.no_grad()
def gaussian_params(entropy_model, positions: Tensor, mins, maxs, return_float: bool = False):
    """The model of every (splat, channel): positions float32 [N, 3] on the device, mins / maxs [C] (the attribute's min-max
    range, as the meta holds it) -> (mu_q int16 [N, C], k uint8 [N, C]), equal to ``gauss_ans_reference.regress_params`` on the
    hash-grid features, element for element.  The hash grid runs as the module runs it (``bound_min`` / ``bound_max`` as held);
    the MLP, the normalisation and the quantisation are ``gs_gauss_ans_params``.  ``return_float`` appends the float32 miu and
    sigma [N, C].  Refused before any launch (ValueError): a module that is not the reference's ``hash_based_estimator`` shape,
    more than 8 channels, a NaN in a hash table (``STE_binary`` maps it to 0, which the one-bit file cannot hold)."""
    c = check_entropy_model(entropy_model)
    if not positions.is_cuda:
        raise RuntimeError("the Gaussian ANS codec runs on the GPU: the positions must be a device tensor (no CPU fallback)")
    if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] < 1:
        raise ValueError(f"positions must be [N, 3], got {tuple(positions.shape)}")
    dev = positions.device
    pr = entropy_model.param_regressor
    if any(p.device != dev for p in pr.parameters()):
        raise RuntimeError("the entropy model and the positions must be on the same device")
    for a in ("xyz", "xy", "xz", "yz"):
        if bool(torch.isnan(getattr(pr.hash_grid, f"encoding_{a}").params).any()):
            raise ValueError(f"encoding_{a} of the entropy model holds a NaN: its sign is 0, which the one-bit table file cannot hold")
    mins_t = torch.as_tensor(mins, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    maxs_t = torch.as_tensor(maxs, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    if mins_t.numel() != c or maxs_t.numel() != c:
        raise ValueError(f"mins / maxs must have {c} entries, got {mins_t.numel()} and {maxs_t.numel()}")
    x = (positions.float() - pr.bound_min) / (pr.bound_max - pr.bound_min)
    feat = pr.hash_grid(x).contiguous()
    n = feat.shape[0]
    w1, b1, w2, b2 = (t.detach().float().contiguous() for t in (pr.mlp_regressor[0].weight, pr.mlp_regressor[0].bias,
                                                                 pr.mlp_regressor[2].weight, pr.mlp_regressor[2].bias))
    mu_q = torch.empty((c, n), dtype=torch.int16, device=dev)
    k = torch.empty((c, n), dtype=torch.uint8, device=dev)
    miu = torch.empty((n, c), dtype=torch.float32, device=dev) if return_float else None
    sigma = torch.empty((n, c), dtype=torch.float32, device=dev) if return_float else None
    with torch.cuda.device(dev):
        B.call("gs_gauss_ans_params", n, c, B.ptr(feat), B.ptr(w1), B.ptr(b1), B.ptr(w2), B.ptr(b2), B.ptr(mins_t), B.ptr(maxs_t),
               B.ptr(_tables(dev)[1]), B.ptr(mu_q), B.ptr(k), B.ptr(miu), B.ptr(sigma), _stream(feat))
    if return_float:
        return mu_q.t(), k.t(), miu, sigma
    return mu_q.t(), k.t()


def _check_model(mu_q: Tensor, k: Tensor, n: int, c: int, dev: torch.device) -> Tuple[Tensor, Tensor]:
    """-> channel-major contiguous (int16 [C, N], uint8 [C, N]); shape, dtype, device and range checked (one read-back)."""
    if not (isinstance(mu_q, Tensor) and isinstance(k, Tensor) and mu_q.is_cuda and k.is_cuda):
        raise RuntimeError("the Gaussian ANS codec runs on the GPU: mu_q and k must be device tensors (no CPU fallback)")
    if tuple(mu_q.shape) != (n, c) or tuple(k.shape) != (n, c):
        raise ValueError(f"the model must be [N, C] = [{n}, {c}], got mu_q {tuple(mu_q.shape)} and k {tuple(k.shape)}")
    if mu_q.dtype != torch.int16 or k.dtype != torch.uint8:
        raise ValueError(f"mu_q must be int16 and k uint8, got {mu_q.dtype} and {k.dtype}")
    mu_cm, k_cm = mu_q.to(dev).t().contiguous(), k.to(dev).t().contiguous()
    lo, hi, k_hi = int(mu_cm.min()), int(mu_cm.max()), int(k_cm.max())
    if lo < 0 or hi > R.MU_Q_MAX or k_hi >= R.N_LEVELS:
        raise ValueError(f"model out of range: mu_q must lie in 0..{R.MU_Q_MAX} and k in 0..{R.N_LEVELS - 1}")
    return mu_cm, k_cm


@torch.no_grad()
def gauss_ans_encode(symbols: Tensor, mu_q: Tensor, k: Tensor, stream_len: int = R.DEFAULT_STREAM_LEN) -> np.ndarray:
    """Encode device symbols uint8 [N, C] against the per-symbol model (mu_q int16, k uint8, both [N, C]) -> the container as a
    numpy uint8 array, byte-identical to ``gauss_ans_reference.encode``."""
    symbols = check_symbols(symbols, MAX_CODER_CHANNELS, "Gaussian ANS codec", stream_len)
    n, c = symbols.shape
    mu_cm, k_cm = _check_model(mu_q, k, n, c, symbols.device)
    table = _tables(symbols.device)[0]
    cm = symbols.t().contiguous()  # channel-major, what the kernel streams through

    def launch(scratch, lengths, states, status, stream):
        B.call("gs_gauss_ans_encode", n, c, stream_len, B.ptr(cm), B.ptr(mu_cm), B.ptr(k_cm), B.ptr(table), B.ptr(scratch),
               scratch.numel(), B.ptr(lengths), B.ptr(states), B.ptr(status), stream)

    offsets, payload = encode_streams(symbols, stream_len, int(B.query("gs_gauss_ans_slot_bytes", stream_len)), launch,
                                      "gs_gauss_ans_encode", "1: model out of range, 2: slot too small")
    return R.build_container(c, stream_len, n, offsets, payload)


@torch.no_grad()
def gauss_ans_decode(blob, mu_q: Tensor, k: Tensor, device="cuda", what: str = "the buffer") -> Tensor:
    """Decode a container (bytes or uint8 array) against the model -> uint8 [N, C] on ``device``, the layout ``dequantize_grid``
    reads.  The container is validated on the host first (ValueError; nothing is launched on a file that is not this project's
    Gaussian container, whose table CRC is another host's, or whose offsets decrease, leave the file or leave a stream fewer than
    4 bytes); the kernel also bounds its own reads."""
    c, stream_len, n, offsets, payload = R.parse_container(blob, what)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the Gaussian ANS codec runs on the GPU (no CPU fallback); gauss_ans_reference.decode is the numpy form")
    if isinstance(mu_q, Tensor) and mu_q.is_cuda:
        dev = mu_q.device
    d_off, d_payload, out = decode_buffers(n, c, stream_len, MAX_CODER_CHANNELS, offsets, payload, dev, what)
    mu_cm, k_cm = _check_model(mu_q, k, n, c, dev)
    table = _tables(dev)[0]
    with torch.cuda.device(dev):
        B.call("gs_gauss_ans_decode", n, c, stream_len, B.ptr(d_payload), d_payload.numel(), B.ptr(d_off), B.ptr(mu_cm), B.ptr(k_cm),
               B.ptr(table), B.ptr(out), _stream(out))
    return out
