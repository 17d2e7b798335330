"""The spacetime colour decoder on the GPU (csrc/stg_decoder.hip; gscodec_studio_amd.dynamic: Sandwich, decode_colors,
render_dynamic(decoder=, rays=)): the forward and the three gradients against tests/golden/stg_decoder.npz (the reference module's
own float64 output) and against the float64 restatement of tests/stg_decoder_reference.py on seeded inputs, at the project's bar of
1e-4 relative L2 per tensor; strided layouts, the halves of the backward and run-to-run identity bit for bit; the wiring into
render_dynamic.

The ReLU mask.  A ReLU decision that differs between float32 and float64 moves one pixel's gradient by O(1), so pixels where a float64
pre-activation of h is within 1e-5 of zero get their upstream gradient zeroed on both sides; at most 0.1 % of the pixels may be."""
import functools

import numpy as np
import pytest
import torch

import stg_decoder_reference as R
from test_stg_decoder_cpu import golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-4
NAMES = ("out", "v_features", "v_w1", "v_w2")


def _module(w1, w2):
    from gscodec_studio_amd.dynamic import getcolormodel

    m = getcolormodel().to(DEV)
    m.load_state_dict({"mlp1.weight": torch.as_tensor(w1), "mlp2.weight": torch.as_tensor(w2)}, strict=True)
    return m


class tuned:
    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        from gscodec_studio_amd import dynamic as D

        self.prev = D._set_decoder_tuning(max_blocks=self.cap)

    def __exit__(self, *a):
        from gscodec_studio_amd import dynamic as D

        D._set_decoder_tuning(**self.prev)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs of one shape (NHWC features / v_out, float32, CPU), the mask and the float64 restatement's results: computed once."""
    f, rays, v = R.seeded_inputs(*shape)
    w1, w2 = R.seeded_weights()
    f, v = f.permute(0, 2, 3, 1).contiguous(), v.permute(0, 2, 3, 1).contiguous()
    keep = R.relu_mask(f, rays, w1)
    v = v * keep.float()
    d = lambda t: t.double()  # noqa: E731
    out = R.decode(d(f), d(rays), d(w1), d(w2))
    v_f, v_w1, v_w2 = R.backward(d(f), d(rays), d(w1), d(w2), d(v))
    return dict(f=f, rays=rays, v=v, w1=w1, w2=w2, masked=1.0 - float(keep.double().mean()), ref=(out, v_f, v_w1, v_w2))


def _run(f, rays, v, w1, w2, grads=(True, True)):
    """(out, v_features, v_w1, v_w2) of decode_colors on the GPU; None where not asked for."""
    from gscodec_studio_amd.dynamic import decode_colors

    f = f.to(DEV).requires_grad_(grads[0])
    w1, w2 = w1.to(DEV).requires_grad_(grads[1]), w2.to(DEV).requires_grad_(grads[1])
    out = decode_colors(f, rays.to(DEV), w1, w2)
    assert out.shape == (*f.shape[:3], 3) and out.is_contiguous()
    if any(grads):
        (out * v.to(DEV)).sum().backward()
    return out.detach(), f.grad, w1.grad, w2.grad


def _errors(tag, got, want):
    errs = {k: R.rel_l2(a.reshape(b.shape), b) for k, a, b in zip(NAMES, got, want)}
    print(f"\n[{tag}] ours vs float64: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    return errs


def test_against_the_reference_fixture():
    fx = golden()
    m = _module(fx["w1"], fx["w2"])
    f = torch.tensor(fx["features"], device=DEV).requires_grad_(True)  # NCHW, as the trainer's permuted view is laid out logically
    out = m(f, torch.tensor(fx["rays"], device=DEV), 0.5)
    assert out.shape == (2, 3, 13, 17) and out.permute(0, 2, 3, 1).is_contiguous()
    (out * torch.tensor(fx["v_out"], device=DEV)).sum().backward()
    got = (out.detach(), f.grad, m.mlp1.weight.grad, m.mlp2.weight.grad)
    assert got[2].shape == (6, 12, 1, 1) and got[3].shape == (3, 6, 1, 1)
    errs = _errors("fixture", got, [fx[k + "_f64"] for k in NAMES])
    e32 = {k: R.rel_l2(fx[k + "_f32"], fx[k + "_f64"]) for k in NAMES}
    print("[fixture] reference float32 vs float64: " + " ".join(f"{k} {e:.2e}" for k, e in e32.items()))
    assert all(e <= BAR for e in errs.values()), errs


@pytest.mark.parametrize("shape,cap", [((1, 5, 7), None), ((2, 37, 53), 2), ((1, 270, 480), None)])
def test_shapes_against_the_float64_restatement(shape, cap):
    """Fewer pixels than a wave; several loop iterations per lane with a ragged tail, two cameras and a cross-workgroup partial sum
    (the workgroup cap forced to 2); 507 workgroups at the default cap."""
    from gscodec_studio_amd import _backend as B

    c = _case(shape)
    print(f"\n[{shape}] masked share {c['masked']:.2e}")
    assert c["masked"] <= R.MASK_SHARE
    if cap is not None:
        assert int(B.query("gs_stg_decode_partial_rows", *shape, cap)) == cap < int(B.query("gs_stg_decode_partial_rows", *shape, 0))
    with tuned(cap):
        got = _run(c["f"], c["rays"], c["v"], c["w1"], c["w2"])
    errs = _errors(f"{shape} cap {cap}", got, c["ref"])
    assert all(e <= BAR for e in errs.values()), errs


def test_strided_layouts_are_read_in_place_bit_for_bit():
    from gscodec_studio_amd.dynamic import decode_colors

    c = _case((2, 37, 53))
    with tuned(2):
        base = _run(c["f"], c["rays"], c["v"], c["w1"], c["w2"])
        v, rays = c["v"].to(DEV), c["rays"].to(DEV)
        # columns 0-8 of a 10-channel render, sliced by the caller and by decode_colors itself
        for sliced in (True, False):
            t = torch.cat((c["f"], torch.full((2, 37, 53, 1), 7.0)), dim=-1).to(DEV).requires_grad_(True)
            w1, w2 = c["w1"].to(DEV).requires_grad_(True), c["w2"].to(DEV).requires_grad_(True)
            out = decode_colors(t[..., :9] if sliced else t, rays, w1, w2)
            (out * v).sum().backward()
            assert torch.equal(out, base[0]) and torch.equal(t.grad[..., :9], base[1]), sliced
            assert not t.grad[..., 9].any()
            assert torch.equal(w1.grad, base[2]) and torch.equal(w2.grad, base[3]), sliced
        # the trainer's call: NHWC render -> permuted NCHW view -> Sandwich.forward -> permuted back
        m = _module(c["w1"], c["w2"])
        render = c["f"].to(DEV).requires_grad_(True)
        out = m(render.permute(0, 3, 1, 2), rays, 0.5)
        assert out.shape == (2, 3, 37, 53)
        out = out.permute(0, 2, 3, 1)
        assert out.is_contiguous()
        (out * v).sum().backward()
        assert torch.equal(out, base[0]) and torch.equal(render.grad, base[1])
        assert torch.equal(m.mlp1.weight.grad, base[2]) and torch.equal(m.mlp2.weight.grad, base[3])
        # a true NCHW tensor (channel stride != 1) and non-contiguous rays are copied, not misread
        nchw = c["f"].permute(0, 3, 1, 2).contiguous().to(DEV)
        rays_t = rays.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        assert not rays_t.is_contiguous()
        with torch.no_grad():
            assert torch.equal(m(nchw, rays_t).permute(0, 2, 3, 1), base[0])


def test_halves_of_the_backward_and_run_to_run_identity():
    c = _case((2, 37, 53))
    args = (c["f"], c["rays"], c["v"], c["w1"], c["w2"])
    with tuned(2):
        full = _run(*args)
        again = _run(*args)
        none = _run(*args, grads=(False, False))
        only_f = _run(*args, grads=(True, False))
        only_w = _run(*args, grads=(False, True))
    assert all(torch.equal(a, b) for a, b in zip(full, again))  # no float atomics: the weight gradients too
    assert torch.equal(none[0], full[0]) and none[1] is None and none[2] is None and none[3] is None
    assert torch.equal(only_f[0], full[0]) and torch.equal(only_f[1], full[1]) and only_f[2] is None and only_f[3] is None
    assert torch.equal(only_w[0], full[0]) and only_w[1] is None
    assert torch.equal(only_w[2], full[2]) and torch.equal(only_w[3], full[3])
    c = _case((1, 270, 480))
    args = (c["f"], c["rays"], c["v"], c["w1"], c["w2"])
    a, b = _run(*args), _run(*args)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------------------------ wiring
W_, H_ = 64, 48
KEYS = ("means", "scales", "quats", "opacities", "trbf_center", "trbf_scale", "motion", "omega", "colors", "features_dir",
        "features_time")


def _scene(n=300, seed=5):
    """A seeded dynamic scene in front of one camera at the origin looking down +z: raw trainer parameters, viewmats, Ks, rays."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    ru = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    raw = {"means": torch.cat(((ru(n, 2) - 0.5) * 3.0, 2.0 + 2.0 * ru(n, 1)), dim=1), "scales": torch.log(0.08 + 0.2 * ru(n, 3)),
           "quats": rn(n, 4), "opacities": rn(n) + 0.5, "trbf_center": ru(n, 1), "trbf_scale": ru(n, 1) - 1.0,
           "motion": 0.02 * rn(n, 9), "omega": 0.1 * rn(n, 4), "colors": rn(n, 3), "features_dir": rn(n, 3), "features_time": rn(n, 3)}
    Ks = torch.tensor([[[50.0, 0.0, W_ / 2], [0.0, 50.0, H_ / 2], [0.0, 0.0, 1.0]]])
    rays = rn(1, 6, H_, W_)
    rays[:, 3:6] = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True)
    return raw, torch.eye(4)[None].to(DEV), Ks.to(DEV), rays.to(DEV)


def _params(raw):
    return {k: torch.nn.Parameter(raw[k].clone().to(DEV)) for k in KEYS}


def test_render_dynamic_applies_the_decoder():
    from gscodec_studio_amd.dynamic import decode_colors, render_dynamic

    raw, vm, Ks, rays = _scene()
    w1, w2 = R.seeded_weights()
    t = 0.4
    # decorated
    P, m = _params(raw), _module(w1, w2)
    rc, ra, info = render_dynamic(P, t, vm, Ks, W_, H_, features="stg", decoder=m, rays=rays, packed=False)
    assert rc.shape == (1, H_, W_, 3) and rc.is_contiguous() and float(ra.detach().max()) > 0.5
    rc.sum().backward()
    # undecorated, decoded by hand
    P2, m2 = _params(raw), _module(w1, w2)
    rc9, ra2, _ = render_dynamic(P2, t, vm, Ks, W_, H_, features="stg", packed=False)
    assert rc9.shape == (1, H_, W_, 9)
    by_hand = decode_colors(rc9, rays, m2.mlp1.weight, m2.mlp2.weight)
    assert torch.equal(rc, by_hand) and torch.equal(ra, ra2)
    by_hand.sum().backward()
    # (the compositing backward adds with float atomics, in another order on every run: not bit for bit)
    errs = {k: R.rel_l2(P[k].grad, P2[k].grad) for k in KEYS if P2[k].grad is not None and float(P2[k].grad.abs().max()) > 0}
    errs["mlp1"], errs["mlp2"] = R.rel_l2(m.mlp1.weight.grad, m2.mlp1.weight.grad), R.rel_l2(m.mlp2.weight.grad, m2.mlp2.weight.grad)
    print("\n[wiring] decorated vs by hand: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert {"means", "colors", "features_dir", "features_time", "mlp1", "mlp2"} <= set(errs)
    assert all(e <= BAR for e in errs.values()), errs
    # the decoder against the float64 restatement on this render
    want = R.decode(rc9.detach().double().cpu(), rays.double().cpu(), w1.double(), w2.double())
    assert R.rel_l2(rc.detach(), want) <= BAR
    # a depth render mode: the depth column follows the three decoded channels unchanged
    with torch.no_grad():
        rcd, _, _ = render_dynamic(_params(raw), t, vm, Ks, W_, H_, features="stg", decoder=m, rays=rays, packed=False, render_mode="RGB+D")
        rc10, _, _ = render_dynamic(_params(raw), t, vm, Ks, W_, H_, features="stg", packed=False, render_mode="RGB+D")
        assert rcd.shape == (1, H_, W_, 4) and rc10.shape == (1, H_, W_, 10)
        assert torch.equal(rcd[..., 3], rc10[..., 9]) and float(rc10[..., 9].max()) > 0
        assert torch.equal(rcd[..., :3], decode_colors(rc10, rays, m.mlp1.weight, m.mlp2.weight))
