"""The appearance module (reference examples/utils.py: AppearanceOptModule, and the two statements the trainer puts behind it,
examples/simple_trainer.py:772-774) restated in plain torch, in whatever dtype its inputs have: the float64 oracle of
tests/test_gpu_appearance.py.  The reference's own class is no float64 oracle: it builds its basis buffer with a dtype-less
``torch.zeros``, so converted to double it still rounds the bases to float32.

    x   = cat(embeds[c], features[n], bases(dirs[c, n] / max(|dirs[c, n]|, 1e-12)) zero-padded to K)
    out = w3 relu(w2 relu(w1 x + b1) + b2) + b3        (+ base[n], through a sigmoid: ``activate``)
"""
import torch

HEAD = ("w1", "b1", "w2", "b2", "w3", "b3")
STATE_KEYS = ("color_head.0.weight", "color_head.0.bias", "color_head.2.weight", "color_head.2.bias", "color_head.4.weight",
              "color_head.4.bias")


def sh_bases(num: int, d):
    """The first ``num`` real spherical-harmonics bases of unit directions d [..., 3] (Sloan's fast evaluation, degree <= 4)."""
    x, y, z = d.unbind(-1)
    one = torch.ones_like(x)
    Y = [0.2820947917738781 * one]
    if num > 1:
        Y += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if num > 4:
        z2 = z * z
        c1, s1 = x * x - y * y, 2 * x * y
        Y += [0.5462742152960395 * s1, -1.092548430592079 * z * y, 0.9461746957575601 * z2 - 0.3153915652525201,
              -1.092548430592079 * z * x, 0.5462742152960395 * c1]
    if num > 9:
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        t0 = -2.285228997322329 * z2 + 0.4570457994644658
        t1 = 1.445305721320277 * z
        Y += [-0.5900435899266435 * s2, t1 * s1, t0 * y, z * (1.865881662950577 * z2 - 1.119528997770346), t0 * x, t1 * c1,
              -0.5900435899266435 * c2]
    if num > 16:
        c3, s3 = x * c2 - y * s2, x * s2 + y * c2
        t0 = z * (-4.683325804901025 * z2 + 2.007139630671868)
        t1 = 3.31161143515146 * z2 - 0.47308734787878
        t2 = -1.770130769779931 * z
        Y += [0.6258357354491763 * s3, t2 * s2, t1 * s1, t0 * y,
              1.984313483298443 * z * Y[12] - 1.006230589874905 * Y[6], t0 * x, t1 * c1, t2 * c2, 0.6258357354491763 * c3]
    return torch.stack(Y[:num], dim=-1)


def inputs(features, embeds, dirs, K: int, sh_degree: int):
    """[C, N, E + F + K]; embeds [C, E] (E may be 0)."""
    C, N = dirs.shape[:2]
    d = dirs / dirs.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    nb = (sh_degree + 1) ** 2
    bases = torch.cat((sh_bases(nb, d), d.new_zeros(C, N, K - nb)), dim=-1)
    return torch.cat((embeds[:, None, :].expand(C, N, -1), features[None].expand(C, N, -1), bases), dim=-1)


def forward(P, features, embeds, dirs, K, sh_degree, base=None, activate=False, pre=False):
    x = inputs(features, embeds, dirs, K, sh_degree)
    z1 = x @ P["w1"].t() + P["b1"]
    z2 = torch.relu(z1) @ P["w2"].t() + P["b2"]
    out = torch.relu(z2) @ P["w3"].t() + P["b3"]
    if base is not None:
        out = out + base[None]
    if activate:
        out = torch.sigmoid(out)
    return (out, z1, z2) if pre else out


def rel_l2(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


def head_of(state, dtype=torch.float64, device="cpu"):
    return {k: torch.as_tensor(state[s]).to(device=device, dtype=dtype) for k, s in zip(HEAD, STATE_KEYS)}


def seeded_inputs(C: int, N: int, F: int = 32, seed: int = 1):
    """features [N, F], dirs [C, N, 3] (lengths 0.5 .. 3), base [N, 3], cotangent [C, N, 3]; float32, CPU."""
    g = torch.Generator().manual_seed(seed)
    features = torch.randn(N, F, generator=g)
    dirs = torch.randn(C, N, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True) * (0.5 + 2.5 * torch.rand(C, N, 1, generator=g))
    base = torch.randn(N, 3, generator=g)
    v_out = torch.randn(C, N, 3, generator=g)
    return features, dirs, base, v_out
