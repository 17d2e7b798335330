"""Dynamic (spacetime) gaussians: temporal slicing at one timestamp.

``temporal_slice`` is the elementwise chain that the reference's dynamic-scene trainer runs in front of
``rasterization()`` (examples/simple_trainer_dyngs.py:506-536; the viewer's copy:
examples/simple_viewer_dyn.py:84-101), as ONE HIP kernel each way (csrc/dynamic.hip) instead of ~25 torch
kernels.  Same inputs as the trainer's local variables: ``opacities`` and ``trbf_scale`` are the
ACTIVATED values (sigmoid / exp are applied by the caller, as in the trainer).  No torch fallback.

``DynamicSlice`` (round 6) hands the same slice to ``rasterization(dynamic=...)``, whose projection kernels then evaluate it in
their load phase (csrc/projection_dyn.hip) -- bit-identical to ``temporal_slice`` followed by ``rasterization``, without the
round trip of means_t / quats_t / opacity_t through HBM; opt-in on top, the trainer's activations (``raw``) and the round
quantizer hooks (``quantize``) ride in the same pass.  ``render_dynamic`` is the dynamic trainer's ``rasterize_splats`` in that form.

The spacetime trainer's colour decoder (reference examples/helper/STG/helper_model.py, applied to the nine-channel render at
examples/simple_trainer_STG.py:578-581) is here too, so that ``from helper.STG.helper_model import getcolormodel, trbfunction``
becomes ``from gscodec_studio_amd.dynamic import getcolormodel, trbfunction``: ``Sandwich`` / ``getcolormodel()`` -- the per-pixel
12 -> 6 -> 3 MLP with the reference's parameters and state-dict keys, one HIP kernel each way (csrc/stg_decoder.hip) --,
``decode_colors`` (its functional form over an NHWC render) and ``trbfunction``.  ``render_dynamic(..., decoder=, rays=)`` applies it.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _backend as B

TEMPORAL_VISIBILITY_THRESHOLD = 0.05  # simple_trainer_dyngs.py:526


class _TemporalSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, motion, quats, omega, opacities, trbf_center, trbf_scale, timestamp):
        if not means.is_cuda:
            raise RuntimeError("temporal_slice: the HIP path needs device tensors (no CPU fallback)")
        ins = [t.contiguous().float() for t in (means, motion, quats, omega, opacities, trbf_center, trbf_scale)]
        n = ins[0].shape[0]
        dev = ins[0].device
        means_t = torch.empty((n, 3), device=dev)
        quats_t = torch.empty((n, 4), device=dev)
        opacity_t = torch.empty((n,), device=dev)
        trbf = torch.empty((n,), device=dev)
        with torch.cuda.device(dev):
            B.call("gs_temporal_slice_fwd", n, *[B.ptr(t) for t in ins], float(timestamp), B.ptr(means_t), B.ptr(quats_t),
                   B.ptr(opacity_t), B.ptr(trbf), torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(*ins)
        ctx.timestamp = float(timestamp)
        ctx.set_materialize_grads(False)
        return means_t, quats_t, opacity_t, trbf

    @staticmethod
    def backward(ctx, v_means_t, v_quats_t, v_opacity_t, v_trbf):
        ins = ctx.saved_tensors
        n = ins[0].shape[0]
        dev = ins[0].device
        need = ctx.needs_input_grad
        outs = [torch.empty_like(t) if need[i] else None for i, t in enumerate(ins)]
        vin = [None if v is None else v.contiguous().float() for v in (v_means_t, v_quats_t, v_opacity_t, v_trbf)]
        with torch.cuda.device(dev):
            B.call("gs_temporal_slice_bwd", n, *[B.ptr(t) for t in ins], ctx.timestamp, *[B.ptr(v) for v in vin],
                   *[B.ptr(o) for o in outs], torch.cuda.current_stream(dev).cuda_stream)
        return (*outs, None)


def temporal_slice(
    means: Tensor,  # [N, 3]
    motion: Tensor,  # [N, 9]  linear | quadratic | cubic coefficients
    quats: Tensor,  # [N, 4]
    omega: Tensor,  # [N, 4]
    opacities: Tensor,  # [N]     activated (sigmoid applied)
    trbf_center: Tensor,  # [N, 1] or [N]
    trbf_scale: Tensor,  # [N, 1] or [N]   activated (exp applied)
    timestamp: float,
    temp_vis_mask: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """Returns (means_t [N,3], quats_t [N,4], opacity_t [N], mask or None).

    ``mask`` (bool [N], ``trbf > 0.05``) is returned when ``temp_vis_mask`` is set; the caller filters the splats with
    it exactly as the trainer does (simple_trainer_dyngs.py:525-535)."""
    N = means.shape[0]
    assert means.shape == (N, 3) and motion.shape == (N, 9) and quats.shape == (N, 4) and omega.shape == (N, 4)
    assert opacities.shape == (N,), opacities.shape
    assert trbf_center.numel() == N and trbf_scale.numel() == N
    means_t, quats_t, opacity_t, trbf = _TemporalSlice.apply(means, motion, quats, omega, opacities, trbf_center.reshape(N),
                                                             trbf_scale.reshape(N), float(timestamp))
    mask = (trbf.detach() > TEMPORAL_VISIBILITY_THRESHOLD) if temp_vis_mask else None
    return means_t, quats_t, opacity_t, mask


# ---------------------------------------------------------------------------------------------------------------------
_RAW_BITS = {"scales": B.const("GS_DYN_RAW_SCALES"), "opacities": B.const("GS_DYN_RAW_OPACITIES"), "trbf_scale": B.const("GS_DYN_RAW_TRBF_SCALE")}
_QUANT_SLOTS = ("scales", "quats", "opacities", "colors")   # bit k of quant_mask
_F4 = ctypes.c_float * 4


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


class DynamicSlice:
    """The temporal part of a set of dynamic gaussians, for ``rasterization(..., dynamic=DynamicSlice(...))``.

    ``rasterization(means, quats, scales, opacities, colors, ..., dynamic=ds)`` equals
    ``rasterization(*temporal_slice(means, ds.motion, quats, ds.omega, opacities, ds.trbf_center, ds.trbf_scale, ds.timestamp)...)``
    (reference examples/simple_trainer_dyngs.py:506-554) with the slice evaluated inside the projection kernels.

    raw       names among ("scales", "opacities", "trbf_scale") (or True for all three) whose tensors are the trainer's RAW
              parameters -- log-scales, opacity logits, log trbf_scale: the exp / sigmoid / exp of dyngs.py:493-505 then runs in the
              kernel too.
    quantize  {"scales" | "quats" | "opacities" | "colors": (lower, upper, bits)}: the attribute goes through the reference's
              round-to-grid STE first (gsplat/compression_simulation/ops.py:57-75): the tensor handed to ``rasterization`` is
              CLAMPED IN PLACE like ``STE.apply``'s input (hand over the parameter itself), quantized values are never
              materialised, the gradient is the identity.  (A quantized attribute that also has an activation must be "raw".)
    min_trbf  the trainer's temporal visibility filter (``temp_vis_mask``, simple_trainer_dyngs.py:526-535: splats whose temporal basis
              ``trbf`` is not above 0.05 are dropped before rasterization): such splats are CULLED by the projection (radius 0, no tiles,
              no gradient) instead of being filtered out of the arrays -- same image, and every ``meta`` tensor keeps its full [C, N]
              shape (the reference re-expands radii / depths / conics / opacities to it afterwards, :557-571).  ``t_vis_mask`` (bool [N])
              holds the mask after the call.
    A plain tuple ``(motion, omega, trbf_center, trbf_scale, timestamp)`` is accepted wherever a DynamicSlice is."""

    def __init__(self, motion: Tensor, omega: Tensor, trbf_center: Tensor, trbf_scale: Tensor, timestamp: float,
                 raw: Union[bool, Sequence[str]] = (), quantize: Optional[Dict[str, Tuple[float, float, int]]] = None,
                 min_trbf: Optional[float] = None):
        self.motion, self.omega, self.trbf_center, self.trbf_scale = motion, omega, trbf_center, trbf_scale
        self.timestamp = float(timestamp)
        self.min_trbf = None if min_trbf is None else float(min_trbf)
        self._alive: Optional[Tensor] = None
        names = tuple(_RAW_BITS) if raw is True else tuple(raw or ())
        assert all(n in _RAW_BITS for n in names), f"raw: names among {tuple(_RAW_BITS)}, got {names}"
        self.raw = names
        self.raw_mask = sum(_RAW_BITS[n] for n in set(names))
        self.quantize = dict(quantize or {})
        assert all(k in _QUANT_SLOTS for k in self.quantize), f"quantize: keys among {_QUANT_SLOTS}, got {tuple(self.quantize)}"
        for k in ("scales", "opacities"):
            assert not (k in self.quantize and k not in names), \
                f"quantize[{k!r}] works on the raw parameter (log-scales / logits): add {k!r} to raw"
        self.quant_mask = sum(1 << _QUANT_SLOTS.index(k) for k in self.quantize)
        lo, hi, rng, qn = [0.0] * 4, [0.0] * 4, [1.0] * 4, [1.0] * 4
        for k, (l_, h_, bits) in self.quantize.items():
            i = _QUANT_SLOTS.index(k)
            # python arithmetic first, then fp32, as torch does with the reference's python-float bounds (ops.py:65-70)
            lo[i], hi[i], rng[i], qn[i] = _f32(l_), _f32(h_), _f32(h_ - l_), _f32(1 / (2 ** bits - 1))
        self._tables = (_F4(*lo), _F4(*hi), _F4(*rng), _F4(*qn))

    @staticmethod
    def of(d) -> "DynamicSlice":
        return d if isinstance(d, DynamicSlice) else DynamicSlice(*d)

    def check(self, N: int) -> None:
        assert self.motion.shape == (N, 9) and self.omega.shape == (N, 4), (self.motion.shape, self.omega.shape)
        assert self.trbf_center.numel() == N and self.trbf_scale.numel() == N, (self.trbf_center.shape, self.trbf_scale.shape)

    def bind(self, quats, scales, opacities, colors, motion, omega, center, tscale):
        """Contiguous fp32 views of the four temporal tensors; refuses a quantized attribute that is not writable in place."""
        for name, t in (("quats", quats), ("scales", scales), ("opacities", opacities), ("colors", colors)):
            if name in self.quantize and t is None:
                raise RuntimeError(f"DynamicSlice: quantize[{name!r}] but no {name} reach the projection "
                                   "(more than three colour channels are quantized by the caller)")
        out = []
        for t in (motion, omega, center, tscale):
            if t.dtype != torch.float32:
                raise RuntimeError(f"DynamicSlice: expected float32 tensors, got {t.dtype}")
            out.append(t if t.is_contiguous() else t.contiguous())
        return tuple(out)

    def c_args(self, dt, fwd_on: Optional[torch.device] = None, N: int = 0):
        """The (motion ... quant_step_norm) run of arguments of gs_projection_rows_dyn_bwd; with ``fwd_on`` (a device) that of
        gs_projection_rows_dyn_fwd, which also takes the temporal visibility threshold and the mask buffer."""
        lo, hi, rng, qn = self._tables
        head = (B.ptr(dt[0]), B.ptr(dt[1]), B.ptr(dt[2]), B.ptr(dt[3]), self.timestamp)
        if fwd_on is not None:
            head += (self.min_trbf_arg(), B.ptr(self.alive_buffer(N, fwd_on)))
        return head + (self.raw_mask, self.quant_mask, ctypes.addressof(lo), ctypes.addressof(hi), ctypes.addressof(rng), ctypes.addressof(qn))

    def min_trbf_arg(self) -> float:
        return -1.0 if self.min_trbf is None else self.min_trbf

    def alive_buffer(self, N: int, device) -> Optional[Tensor]:
        """The uint8 [N] buffer the forward writes the temporal visibility into (None without ``min_trbf``)."""
        if self.min_trbf is None:
            return None
        self._alive = torch.empty((N,), dtype=torch.uint8, device=device)
        return self._alive

    @property
    def t_vis_mask(self) -> Optional[Tensor]:
        return None if self._alive is None else self._alive.bool()

    # -- the same chain through the stand-alone operators: every route the fused kernels do not cover (packed, distributed, SH colours,
    # covars, camera-pose gradients) and the reference the fused route is tested against
    def apply_unfused(self, means, quats, scales, opacities, colors):
        """-> (means_t, quats_t, scales, opacity_t, colors) for a plain ``rasterization`` call: STE hooks (in-place clamp), activations,
        ``temporal_slice``."""
        from .compression_simulation.ops import STE

        def q(name, t, act):
            if name in self.quantize:
                lo, hi, bits = self.quantize[name]
                return STE.apply(t, bits, lo, hi, act)
            if act == 1:
                return torch.exp(t)
            if act == 2:
                return torch.sigmoid(t)
            return t

        quats = q("quats", quats, 0)
        scales = q("scales", scales, 1 if "scales" in self.raw else 0)
        opacities = q("opacities", opacities, 2 if "opacities" in self.raw else 0)
        if colors is not None and "colors" in self.quantize:
            colors = q("colors", colors, 0)
        tscale = torch.exp(self.trbf_scale) if "trbf_scale" in self.raw else self.trbf_scale
        means_t, quats_t, opacity_t, trbf = _TemporalSlice.apply(means, self.motion, quats, self.omega, opacities,
                                                                 self.trbf_center.reshape(-1), tscale.reshape(-1), self.timestamp)
        if self.min_trbf is not None:
            # (the stand-alone route cannot drop the splats -- meta keeps its [C, N] shape -- so they are made invisible instead: an
            # opacity of zero composites nothing and receives no gradient, like the trainer's filter)
            self._alive = (trbf.detach() > self.min_trbf).to(torch.uint8)
            opacity_t = opacity_t * self._alive.to(opacity_t.dtype)
        return means_t, quats_t, scales, opacity_t, colors


_STG_PARTS = ("colors", "features_dir", "features_time")  # bit p of gs_stg_features_fwd's quant_mask
_F3 = ctypes.c_float * 3


class _StgFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, features_dir, features_time, trbf_center, timestamp, quantize):
        if not colors.is_cuda:
            raise RuntimeError("stg_features: the HIP path needs device tensors (no CPU fallback)")
        n = colors.shape[0]
        for name, t in zip(_STG_PARTS, (colors, features_dir, features_time)):
            assert t.shape == (n, 3), (name, t.shape)
            if name in quantize and not (t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError(f"stg_features: quantize[{name!r}] clamps the tensor in place -- hand over the contiguous float32 parameter")
        parts = [t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float() for t in (colors, features_dir, features_time)]
        center = trbf_center.detach().reshape(-1).contiguous().float()
        assert center.numel() == n, trbf_center.shape
        lo, hi, rng, qn = [0.0] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3
        mask = 0
        for k, (l_, h_, bits) in quantize.items():
            i = _STG_PARTS.index(k)
            mask |= 1 << i
            lo[i], hi[i], rng[i], qn[i] = _f32(l_), _f32(h_), _f32(h_ - l_), _f32(1 / (2 ** bits - 1))
        out = torch.empty((n, 9), dtype=torch.float32, device=colors.device)
        with torch.cuda.device(colors.device):
            B.call("gs_stg_features_fwd", n, *[B.ptr(t) for t in parts], B.ptr(center), float(timestamp), mask,
                   _F3(*lo), _F3(*hi), _F3(*rng), _F3(*qn), B.ptr(out), torch.cuda.current_stream(colors.device).cuda_stream)
        ctx.save_for_backward(center)
        ctx.timestamp = float(timestamp)
        return out

    @staticmethod
    def backward(ctx, v_out):
        (center,) = ctx.saved_tensors
        n = center.shape[0]
        need = ctx.needs_input_grad
        v_out = v_out.contiguous().float()
        grads = [torch.empty((n, 3), dtype=torch.float32, device=center.device) if need[i] else None for i in range(3)]
        with torch.cuda.device(center.device):
            B.call("gs_stg_features_bwd", n, B.ptr(v_out), B.ptr(center), ctx.timestamp, *[B.ptr(g) for g in grads],
                   torch.cuda.current_stream(center.device).cuda_stream)
        return (*grads, None, None, None)


def stg_features(colors: Tensor, features_dir: Tensor, features_time: Tensor, trbf_center: Tensor, timestamp: float,
                 quantize: Optional[Dict[str, Tuple[float, float, int]]] = None) -> Tensor:
    """The spacetime trainer's nine colour channels ``torch.cat((colors, features_dir, tforpoly * features_time), dim=1)`` with
    ``tforpoly = (timestamp - trbf_center).detach()`` (reference examples/simple_trainer_STG.py:506-551) in one kernel each way
    (``gs_stg_features_fwd`` / ``_bwd``, csrc/dynamic.hip) -- same values bit for bit, no [N,9] copy by ``cat``, no split + copies by
    autograd on the way back.  ``quantize``: {"colors" | "features_dir" | "features_time": (lower, upper, bits)} runs that part through
    the compression simulation's round-to-grid STE first (the tensor is CLAMPED IN PLACE like ``STE.apply``'s input; identity gradient)."""
    quantize = dict(quantize or {})
    assert all(k in _STG_PARTS for k in quantize), f"quantize: keys among {_STG_PARTS}, got {tuple(quantize)}"
    return _StgFeatures.apply(colors, features_dir, features_time, trbf_center, timestamp, quantize)


# ---------------------------------------------------------------------------------------------------------------------
# The spacetime colour decoder  (csrc/stg_decoder.hip)
_DECODER_TUNING = {"max_blocks": 0}  # cap of the kernels' grid in workgroups; 0 = the library's default


def _set_decoder_tuning(**kv) -> dict:
    """Set tuning values (key: max_blocks; ``None`` / 0 = default) for the decoder calls that FOLLOW (a forward's backward reads the
    value again); returns the previous values.  For tests: a small cap forces the grid-stride loop at a small shape."""
    prev = dict(_DECODER_TUNING)
    for k, v in kv.items():
        assert k in _DECODER_TUNING, k
        _DECODER_TUNING[k] = 0 if v is None else int(v)
    return prev


def _pixel_strided(f9: Tensor) -> Tuple[Tensor, int]:
    """[C, H, W, 9] as the kernels read it, with its pixel stride: channel stride 1 and ONE pixel stride over the whole [C H W] run
    (a contiguous copy otherwise)."""
    C, H, W, _ = f9.shape
    ps = f9.stride(2) if W > 1 else (f9.stride(1) if H > 1 else max(f9.stride(0), 9))
    ok = f9.stride(3) == 1 and ps >= 9 and (H == 1 or f9.stride(1) == W * ps) and (C == 1 or f9.stride(0) == H * W * ps)
    return (f9, ps) if ok else (f9.contiguous(), 9)


class _DecodeColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f9, rays, w1, w2):
        C, H, W, _ = f9.shape
        f9, ps = _pixel_strided(f9)
        if not (rays.stride(3) == 1 and (H == 1 or rays.stride(2) == W)):
            rays = rays.contiguous()
        w1c, w2c = w1.contiguous(), w2.contiguous()
        out = torch.empty((C, H, W, 3), dtype=torch.float32, device=f9.device)
        ctx.geo = (C, H, W, ps, rays.stride(0), rays.stride(1))
        with torch.cuda.device(f9.device):
            B.call("gs_stg_decode_fwd", C, H, W, B.ptr(f9), ctx.geo[3], B.ptr(rays), ctx.geo[4], ctx.geo[5], B.ptr(w1c), B.ptr(w2c),
                   _DECODER_TUNING["max_blocks"], B.ptr(out), torch.cuda.current_stream(f9.device).cuda_stream)
        ctx.save_for_backward(f9, rays, w1c, w2c)
        ctx.w_shapes = (w1.shape, w2.shape)
        return out

    @staticmethod
    def backward(ctx, v_out):
        f9, rays, w1c, w2c = ctx.saved_tensors
        C, H, W, ps, rs_cam, rs_ch = ctx.geo
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        if not (need_f or need_w):
            return None, None, None, None
        dev = f9.device
        v_out = v_out.contiguous().float()
        cap = _DECODER_TUNING["max_blocks"]
        v_f = torch.empty((C, H, W, 9), dtype=torch.float32, device=dev) if need_f else None
        partials = None
        if need_w:
            partials = torch.empty((int(B.query("gs_stg_decode_partial_rows", C, H, W, cap)), 90), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            B.call("gs_stg_decode_bwd", C, H, W, B.ptr(f9), ps, B.ptr(rays), rs_cam, rs_ch, B.ptr(w1c), B.ptr(w2c), B.ptr(v_out), cap,
                   B.ptr(v_f), B.ptr(partials), torch.cuda.current_stream(dev).cuda_stream)
        v_w1 = v_w2 = None
        if need_w:
            sums = partials.sum(dim=0)  # (one row per workgroup, added here in torch's fixed order: no float atomics anywhere)
            v_w1 = sums[:72].reshape(ctx.w_shapes[0]) if ctx.needs_input_grad[2] else None
            v_w2 = sums[72:].reshape(ctx.w_shapes[1]) if ctx.needs_input_grad[3] else None
        return v_f, None, v_w1, v_w2


def decode_colors(features: Tensor, rays: Tensor, w1: Tensor, w2: Tensor) -> Tensor:
    """The spacetime colour decoder over an NHWC render: ``features`` ``[C, H, W, >= 9]`` (the first nine channels are used and read in
    place, e.g. a 10-channel ``RGB+D`` render or the permuted NCHW view the trainer makes), ``rays`` ``[C, 6, H, W]`` (origin, unit
    direction; no gradient), ``w1`` = ``mlp1.weight`` ``[6, 12(, 1, 1)]``, ``w2`` = ``mlp2.weight`` ``[3, 6(, 1, 1)]`` -> ``[C, H, W, 3]``:
    ``sigmoid(features[..., :3] + w2 relu(w1 cat(features[..., 3:9], rays)))`` per pixel.  One kernel forward, one backward
    (gradients of the features and of both weights; the weights' are bit-identical from run to run)."""
    for name, t in (("features", features), ("rays", rays), ("w1", w1), ("w2", w2)):
        if not isinstance(t, Tensor) or t.dtype != torch.float32:
            raise ValueError(f"decode_colors: {name} must be a float32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
    if features.dim() != 4 or features.shape[-1] < 9 or features.numel() == 0:
        raise ValueError(f"decode_colors: features must be a non-empty [C, H, W, >= 9] tensor (got shape {tuple(features.shape)})")
    C, H, W, _ = features.shape
    if tuple(rays.shape) != (C, 6, H, W):
        raise ValueError(f"decode_colors: rays must be [C, 6, H, W] = {(C, 6, H, W)} (got shape {tuple(rays.shape)})")
    if w1.numel() != 72 or tuple(w1.shape[:2]) != (6, 12) or w2.numel() != 18 or tuple(w2.shape[:2]) != (3, 6):
        raise ValueError(f"decode_colors: w1 must be [6, 12(, 1, 1)] and w2 [3, 6(, 1, 1)] (got {tuple(w1.shape)}, {tuple(w2.shape)})")
    if rays.requires_grad:
        raise NotImplementedError("decode_colors: rays requires a gradient, but the decoder has none for the rays (detach it)")
    if C * H * W >= 2 ** 32:
        raise ValueError(f"decode_colors: {tuple(features.shape)} has more than 2^32 - 1 pixels")
    for name, t in (("features", features), ("rays", rays), ("w1", w1), ("w2", w2)):
        if not t.is_cuda:
            raise RuntimeError(f"decode_colors: the HIP path needs device tensors, {name} is on {t.device} (no CPU fallback)")
        if t.device != features.device:
            raise RuntimeError(f"decode_colors: features and {name} are on different devices ({features.device}, {t.device})")
    return _DecodeColors.apply(features[..., :9], rays, w1, w2)


class Sandwich(nn.Module):
    """The spacetime trainer's colour decoder with the reference module's parameters: ``mlp1`` (12 -> 6) and ``mlp2`` (6 -> 3), 1x1
    convolutions without bias, created in that order -- the same ``state_dict`` keys, shapes and seeded initialisation, so
    checkpoints load both ways with ``strict=True``.  ``dim`` and ``outdim`` are accepted and, as in the reference, unused."""

    def __init__(self, dim: int = 9, outdim: int = 3, bias: bool = False):
        super().__init__()
        if bias:
            raise NotImplementedError("Sandwich: bias=True is not implemented (the kernels are bias-free, as getcolormodel() is)")
        self.mlp1 = nn.Conv2d(12, 6, kernel_size=1, bias=False)
        self.mlp2 = nn.Conv2d(6, 3, kernel_size=1, bias=False)

    def forward(self, input: Tensor, rays: Tensor, time=None) -> Tensor:  # noqa: A002
        """``input`` ``[C, 9, H, W]`` (the trainer's permuted view of the NHWC render is read in place), ``rays`` ``[C, 6, H, W]`` ->
        ``[C, 3, H, W]``, a permuted view of the kernel's NHWC output: the trainer's ``.permute(0, 2, 3, 1)`` that follows is
        contiguous.  ``time`` is unused, as in the reference."""
        if not isinstance(input, Tensor) or input.dim() != 4 or input.shape[1] != 9:
            raise ValueError(f"Sandwich: input must be [C, 9, H, W] (got shape {tuple(getattr(input, 'shape', ()))})")
        return decode_colors(input.permute(0, 2, 3, 1), rays, self.mlp1.weight, self.mlp2.weight).permute(0, 3, 1, 2)


def getcolormodel() -> Sandwich:
    return Sandwich(9, 3)


def trbfunction(x: Tensor) -> Tensor:
    """The temporal radial basis ``exp(-x^2)`` (plain torch)."""
    return torch.exp(-(x * x))


def render_dynamic(splats: Dict[str, Tensor], timestamp: float, viewmats: Tensor, Ks: Tensor, width: int, height: int,
                   compression_sim=None, step: int = 0, features: str = "colors", temp_vis_mask: bool = False, decoder=None,
                   rays: Optional[Tensor] = None, **kwargs):
    """The dynamic trainer's ``rasterize_splats`` (reference examples/simple_trainer_dyngs.py:463-577, compression_sim on or off) on
    the fused route: ``splats`` is the trainer's RAW parameter dict (means, scales (log), quats, opacities (logits), trbf_center,
    trbf_scale (log), motion, omega, colors [, features_dir, features_time]); returns ``(render_colors, render_alphas, info)``.

    With ``compression_sim`` (an ``STGCompressionSimulation`` in "round" mode) the hooks of scales / quats / opacities / colors run
    inside the projection kernel (parameters clamped in place, as the hooks do) unless the step needs their quantized values for the
    bits estimator (``step > entropy_steps[name]``) -- those attributes, and every other mode of the simulation, go through
    ``simulate_compression`` as usual and only the activations + slice are fused.  ``features="stg"`` renders the spacetime trainer's
    nine channels cat(colors, features_dir, tau * features_time) (examples/simple_trainer_STG.py:506-551).
    ``temp_vis_mask`` (the trainer's option, dyngs.py:137, 526-571): splats whose temporal basis is <= 0.05 at this timestamp are culled
    by the projection; ``info["t_vis_mask"]`` is the mask and the per-gaussian ``info`` tensors are full-size, as the reference leaves them
    (its ``info["means2d"]`` alone stays compacted to the masked subset: here it is [C, N, 2] like the rest).
    ``decoder`` (a ``Sandwich``, with ``features="stg"``) and ``rays`` ``[C, 6, H, W]``: the nine rendered channels go through the colour
    decoder (examples/simple_trainer_STG.py:578-581) and ``render_colors`` is the decoded ``[C, H, W, 3]``; with a depth render mode the
    depth column follows unchanged.
    -> also returns ``esti_bits`` of the hooks that ran outside as ``info["esti_bits"]``."""
    from .rendering import rasterization

    if decoder is not None and (features != "stg" or rays is None):
        raise ValueError('render_dynamic: decoder needs features="stg" and rays [C, 6, H, W]')
    P = dict(splats)
    esti_bits = {}
    quantize = {}
    raw = ["scales", "opacities", "trbf_scale"]
    sim = compression_sim
    if sim is not None:
        in_kernel = []
        if getattr(sim, "q_type", None) == "round":
            # (the nine-channel render takes its three colour parts through stg_features: their hooks ride in THAT kernel)
            for name in _QUANT_SLOTS + (("features_dir", "features_time") if (features == "stg" and P["colors"].is_cuda) else ()):
                if name == "colors" and features != "colors" and not P["colors"].is_cuda:
                    continue
                needs_bits = (sim.entropy_model_enable and sim.entropy_model_option.get(name, False)
                              and step > sim.entropy_steps.get(name, -1) and sim.entropy_models.get(name) is not None)
                if sim.simulation_option.get(name, False) and sim.bds.get(name) is not None and not needs_bits and name in P:
                    in_kernel.append(name)
        rest = {k: v for k, v in P.items() if k not in in_kernel and sim.simulation_option.get(k, False)}
        if rest:
            new, bits = sim.simulate_compression(rest, step)
            P.update(new)
            esti_bits.update(bits)
        for name in in_kernel:
            lo, hi = sim.bds[name]
            quantize[name] = (lo, hi, sim.q_bitwidth[name])
    if features == "stg":
        if P["colors"].is_cuda:
            colors = stg_features(P["colors"], P["features_dir"], P["features_time"], P["trbf_center"], timestamp,
                                  quantize={k: quantize.pop(k) for k in _STG_PARTS if k in quantize})
        else:
            tau = (float(timestamp) - P["trbf_center"]).detach()
            colors = torch.cat((P["colors"], P["features_dir"], tau * P["features_time"]), dim=1)
    else:
        colors = P["colors"]
    ds = DynamicSlice(P["motion"], P["omega"], P["trbf_center"], P["trbf_scale"], timestamp, raw=raw, quantize=quantize,
                      min_trbf=TEMPORAL_VISIBILITY_THRESHOLD if temp_vis_mask else None)
    rc, ra, info = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], colors, viewmats, Ks, width, height,
                                 dynamic=ds, **kwargs)
    info["esti_bits"] = esti_bits
    if temp_vis_mask:
        info["t_vis_mask"] = ds.t_vis_mask
    if decoder is not None:
        decoded = decoder(rc[..., :9].permute(0, 3, 1, 2), rays, timestamp).permute(0, 2, 3, 1)
        rc = decoded if rc.shape[-1] == 9 else torch.cat((decoded, rc[..., 9:]), dim=-1)
    return rc, ra, info
