"""The static trainer's appearance module (``--app_opt``): reference examples/utils.py ``AppearanceOptModule``, called at
examples/simple_trainer.py:766-774, with everything between the parameters and the ``[C, N, 3]`` colours in ONE HIP kernel each way
(csrc/appearance.hip, on the matrix cores) instead of a ``[C, N, 64]`` cat, a ``[C, N, 16]`` basis tensor, three saved
``[C, N, 64]`` activations and five vendor-BLAS launches each way.

``from gscodec_studio_amd.appearance import AppearanceOptModule`` in place of ``from utils import AppearanceOptModule``: same
constructor, same ``state_dict`` keys, shapes and seeded initialisation, same ``forward(features, embed_ids, dirs, sh_degree)``.
The fused form of the trainer's lines 767-774 is ``module.colors(features, embed_ids, means, camtoworlds, sh_degree,
base=splats["colors"])`` = ``sigmoid(forward(features, embed_ids, means[None] - camtoworlds[:, None, :3, 3], sh_degree) + base)``
without the ``[C, N, 3]`` direction tensor.  The embedding lookup stays in torch (``[C, E]``): its backward handles repeated ids and
gives the dense gradient that the trainer's ``Adam(weight_decay=...)`` expects.  No torch fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from . import _backend as B

HIDDEN = 64          # mlp_width of the kernels
MAX_FEATURES = 96    # csrc/appearance.hip: three feature tiles of 32 columns
MAX_INPUT = 128

_APPEARANCE_TUNING = {"max_blocks": 0}  # cap of the kernels' grid in workgroups; 0 = the library's default


def _set_appearance_tuning(**kv) -> dict:
    """Set tuning values (key: max_blocks; ``None`` / 0 = default) for the calls that FOLLOW (a forward's backward reads the value
    again); returns the previous values.  For tests: a small cap makes one workgroup loop over tiles at a small shape."""
    prev = dict(_APPEARANCE_TUNING)
    for k, v in kv.items():
        assert k in _APPEARANCE_TUNING, k
        _APPEARANCE_TUNING[k] = 0 if v is None else int(v)
    return prev


class _Appearance(torch.autograd.Function):
    """features [N, F], embeds [C, E] or None, geometry (dirs [C, N, 3], or means [N, 3] and cam_centers [C, 3]), the six weights,
    base [N, 3] or None -> colours [C, N, 3]."""

    @staticmethod
    def forward(ctx, features, embeds, dirs, means, cams, w1, b1, w2, b2, w3, b3, base, K, num_bases, activate):
        dev = features.device
        N, F = features.shape
        C = dirs.shape[0] if dirs is not None else cams.shape[0]
        E = w1.shape[1] - F - K
        ins = [None if t is None else t.detach().contiguous()
               for t in (features, embeds, dirs, means, cams, w1, b1, w2, b2, w3, b3, base)]
        out = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
        ctx.geo = (N, C, F, E, K, num_bases, int(bool(activate)))
        with torch.cuda.device(dev):
            B.call("gs_appearance_fwd", N, C, F, E, K, num_bases, *[B.ptr(t) for t in ins], int(bool(activate)),
                   _APPEARANCE_TUNING["max_blocks"], B.ptr(out), torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(*[t for t in ins if t is not None])
        ctx.present = [t is not None for t in ins]
        return out

    @staticmethod
    def backward(ctx, v_out):
        saved = iter(ctx.saved_tensors)
        ins = [next(saved) if p else None for p in ctx.present]
        features, embeds, dirs, means, cams, w1, b1, w2, b2, w3, b3, base = ins
        N, C, F, E, K, num_bases, activate = ctx.geo
        dev = features.device
        need = ctx.needs_input_grad
        v_out = v_out.contiguous().float()
        cap = _APPEARANCE_TUNING["max_blocks"]

        def new(shape, wanted):
            return torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None

        v_features = new((N, F), need[0])
        v_dirs = new((C, N, 3), dirs is not None and need[2])
        # (without bases above the constant one the direction has no gradient: the kernel skips it, the buffer is zero)
        v_means = None
        if dirs is None and need[3]:
            v_means = torch.zeros((N, 3), dtype=torch.float32, device=dev) if num_bases == 1 else new((N, 3), True)
        if v_dirs is not None and num_bases == 1:
            v_dirs.zero_()
        v_base = new((N, 3), base is not None and need[11])
        rows = int(B.query("gs_appearance_partial_rows", N, F, E, K, cap))
        cols = int(B.query("gs_appearance_partial_cols", C, F, K))
        partials = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            B.call("gs_appearance_bwd", N, C, F, E, K, num_bases, *[B.ptr(t) for t in ins], activate, B.ptr(v_out), cap,
                   B.ptr(v_features), B.ptr(v_dirs), B.ptr(v_means), B.ptr(v_base), B.ptr(partials),
                   torch.cuda.current_stream(dev).cuda_stream)
        # one row per wave, added here in torch's fixed order: no float atomics anywhere
        sums = partials.sum(dim=0)
        o = 0
        parts = []
        for n in (HIDDEN * (F + K), HIDDEN * HIDDEN, 3 * HIDDEN, HIDDEN, 4, C * HIDDEN):
            parts.append(sums[o:o + n])
            o += n
        v_w1x, v_w2, v_w3, v_b2, v_b3, d_pre = parts
        d_pre = d_pre.reshape(C, HIDDEN)  # gradient of the per-camera pre-activation w1[:, :E] embeds[c] + b1
        v_embeds = None
        v_w1e = torch.zeros((HIDDEN, E), dtype=torch.float32, device=dev)
        if embeds is not None and E:
            v_w1e = d_pre.t() @ embeds
            if need[1]:
                v_embeds = d_pre @ w1[:, :E]
        v_w1 = torch.cat((v_w1e, v_w1x.reshape(HIDDEN, F + K)), dim=1) if need[5] else None
        return (v_features, v_embeds, v_dirs, v_means, None,
                v_w1, d_pre.sum(dim=0) if need[6] else None, v_w2.reshape(HIDDEN, HIDDEN) if need[7] else None,
                v_b2 if need[8] else None, v_w3.reshape(3, HIDDEN) if need[9] else None, v_b3[:3] if need[10] else None,
                v_base, None, None, None)


class AppearanceOptModule(nn.Module):
    """Appearance optimization module: ``embeds`` (``Embedding(n, embed_dim)``) and ``color_head`` (``Linear`` / ``ReLU`` ... ``Linear(., 3)``)
    created in the reference's order -- the same ``state_dict`` keys (``embeds.weight``, ``color_head.{0,2,4}.{weight,bias}``), shapes and
    seeded initialisation, so checkpoints load both ways with ``strict=True``.  The kernels cover ``mlp_width = 64``, ``mlp_depth = 2``,
    ``sh_degree <= 4``, ``1 <= feature_dim <= 96`` and ``embed_dim + feature_dim + (sh_degree + 1)^2 <= 128``."""

    def __init__(self, n: int, feature_dim: int, embed_dim: int = 16, sh_degree: int = 3, mlp_width: int = 64, mlp_depth: int = 2):
        super().__init__()
        K = (sh_degree + 1) ** 2
        if mlp_width != HIDDEN or mlp_depth != 2:
            raise NotImplementedError(f"AppearanceOptModule: the kernels cover mlp_width = 64 and mlp_depth = 2 "
                                      f"(got {mlp_width}, {mlp_depth})")
        if not 0 <= sh_degree <= 4:
            raise NotImplementedError(f"AppearanceOptModule: sh_degree must be in 0..4 (got {sh_degree})")
        if not (1 <= feature_dim <= MAX_FEATURES and embed_dim >= 0 and embed_dim + feature_dim + K <= MAX_INPUT):
            raise NotImplementedError(f"AppearanceOptModule: the kernels cover 1 <= feature_dim <= {MAX_FEATURES} and embed_dim + "
                                      f"feature_dim + (sh_degree + 1)^2 <= {MAX_INPUT} (got {feature_dim}, {embed_dim}, {K})")
        self.embed_dim = embed_dim
        self.sh_degree = sh_degree
        self.feature_dim = feature_dim
        self.embeds = nn.Embedding(n, embed_dim)
        layers = [nn.Linear(embed_dim + feature_dim + K, mlp_width), nn.ReLU(inplace=True)]
        for _ in range(mlp_depth - 1):
            layers += [nn.Linear(mlp_width, mlp_width), nn.ReLU(inplace=True)]
        layers.append(nn.Linear(mlp_width, 3))
        self.color_head = nn.Sequential(*layers)

    # -- checks shared by both forms: everything is refused before a launch
    def _check(self, who: str, features, sh_degree: int, tensors) -> list:
        K = (self.sh_degree + 1) ** 2
        params = [("color_head.%d.%s" % (i, k), getattr(self.color_head[i], k)) for i in (0, 2, 4) for k in ("weight", "bias")]
        for name, t in tensors + params:
            if not isinstance(t, Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{who}: {name} must be a float32 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
        if features.dim() != 2 or features.shape[1] != self.feature_dim or features.shape[0] == 0:
            raise ValueError(f"{who}: features must be a non-empty [N, {self.feature_dim}] tensor (got shape {tuple(features.shape)})")
        if not isinstance(sh_degree, int) or not 0 <= sh_degree <= self.sh_degree:
            raise ValueError(f"{who}: sh_degree must be an integer in 0..{self.sh_degree} (got {sh_degree!r})")
        shapes = ((HIDDEN, self.embed_dim + self.feature_dim + K), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (3, HIDDEN), (3,))
        for (name, t), shape in zip(params, shapes):
            if tuple(t.shape) != shape:
                raise NotImplementedError(f"{who}: {name} has shape {tuple(t.shape)}, the kernels cover {shape}")
        return params

    @staticmethod
    def _check_devices(who: str, tensors) -> None:
        for name, t in tensors:
            if not t.is_cuda:
                raise RuntimeError(f"{who}: the HIP path needs device tensors, {name} is on {t.device} (no CPU fallback)")
            if t.device != tensors[0][1].device:
                raise RuntimeError(f"{who}: {tensors[0][0]} and {name} are on different devices ({tensors[0][1].device}, {t.device})")

    def _embeds(self, who: str, embed_ids, C: int) -> Optional[Tensor]:
        if embed_ids is None or self.embed_dim == 0:
            return None  # a zero embedding / no embedding columns
        if embed_ids.dim() != 1 or embed_ids.shape[0] != C:
            raise ValueError(f"{who}: embed_ids must be [C] = [{C}] (got shape {tuple(embed_ids.shape)})")
        return self.embeds(embed_ids)  # [C, E], torch: repeated ids and the dense gradient are Embedding's business

    def _head(self):
        h = self.color_head
        return h[0].weight, h[0].bias, h[2].weight, h[2].bias, h[4].weight, h[4].bias

    def forward(self, features: Tensor, embed_ids: Optional[Tensor], dirs: Tensor, sh_degree: int) -> Tensor:
        """features [N, feature_dim], embed_ids int [C] or None (a zero embedding), dirs [C, N, 3] (not normalised) -> the raw
        colours [C, N, 3]: the reference's forward, one kernel each way."""
        who = "AppearanceOptModule.forward"
        tensors = [("features", features), ("dirs", dirs)]
        params = self._check(who, features, sh_degree, tensors)
        N = features.shape[0]
        if dirs.dim() != 3 or dirs.shape[1:] != (N, 3) or dirs.shape[0] == 0:
            raise ValueError(f"{who}: dirs must be [C, N, 3] with N = {N} (got shape {tuple(dirs.shape)})")
        self._check_devices(who, tensors + params)
        emb = self._embeds(who, embed_ids, dirs.shape[0])
        return _Appearance.apply(features, emb, dirs, None, None, *self._head(), None, (self.sh_degree + 1) ** 2,
                                 (sh_degree + 1) ** 2, False)

    def colors(self, features: Tensor, embed_ids: Optional[Tensor], means: Tensor, camtoworlds: Tensor, sh_degree: int,
               base: Optional[Tensor] = None) -> Tensor:
        """The trainer's lines 767-774 in one call: ``sigmoid(forward(features, embed_ids, means[None] - camtoworlds[:, None, :3, 3],
        sh_degree) + base)`` -> [C, N, 3], for ``rasterization(colors=..., sh_degree=None)``.  means [N, 3], camtoworlds [C, 4, 4] (no
        gradient), base [N, 3] (``splats["colors"]``) or None.  Gradients go to features, means, base, the embeddings and the head."""
        who = "AppearanceOptModule.colors"
        tensors = [("features", features), ("means", means), ("camtoworlds", camtoworlds)] + ([("base", base)] if base is not None else [])
        params = self._check(who, features, sh_degree, tensors)
        N = features.shape[0]
        if tuple(means.shape) != (N, 3):
            raise ValueError(f"{who}: means must be [N, 3] with N = {N} (got shape {tuple(means.shape)})")
        if camtoworlds.dim() != 3 or camtoworlds.shape[1:] != (4, 4) or camtoworlds.shape[0] == 0:
            raise ValueError(f"{who}: camtoworlds must be [C, 4, 4] (got shape {tuple(camtoworlds.shape)})")
        if base is not None and tuple(base.shape) != (N, 3):
            raise ValueError(f"{who}: base must be [N, 3] with N = {N} (got shape {tuple(base.shape)})")
        if camtoworlds.requires_grad:
            raise NotImplementedError(f"{who}: camtoworlds requires a gradient, which the fused form does not produce: use the drop-in "
                                      "form, forward(features, embed_ids, means[None] - camtoworlds[:, None, :3, 3], sh_degree)")
        self._check_devices(who, tensors + params)
        emb = self._embeds(who, embed_ids, camtoworlds.shape[0])
        cams = camtoworlds[:, :3, 3].detach().contiguous()
        return _Appearance.apply(features, emb, None, means, cams, *self._head(), base, (self.sh_degree + 1) ** 2,
                                 (sh_degree + 1) ** 2, True)
