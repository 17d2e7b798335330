"""The spacetime colour decoder without a GPU: the float64 restatement of tests/stg_decoder_reference.py reproduces
tests/golden/stg_decoder.npz -- the reference module's own outputs and gradients -- to 1e-12 (its float64 arrays) and 1e-5 (its
float32 arrays); ``Sandwich`` has the reference's state-dict keys, shapes and seeded initialisation and loads the fixture's weights
with strict=True; what it does not cover is refused; the native entry points are part of the C ABI and answer bad arguments before
any launch.  The GPU tests use the restatement as their oracle."""
import os

import numpy as np
import pytest
import torch

import stg_decoder_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stg_decoder.npz")


def golden():
    return dict(np.load(GOLDEN))


def restated(fx, dtype=torch.float64):
    """(out, v_features, v_w1, v_w2) of the restatement on the fixture's inputs, NCHW like the fixture."""
    T = lambda k: torch.tensor(fx[k], dtype=dtype)  # noqa: E731
    f, v = T("features").permute(0, 2, 3, 1), T("v_out").permute(0, 2, 3, 1)
    out = R.decode(f, T("rays"), T("w1"), T("w2"))
    v_f, v_w1, v_w2 = R.backward(f, T("rays"), T("w1"), T("w2"), v)
    return {"out": out.permute(0, 3, 1, 2), "v_features": v_f.permute(0, 3, 1, 2), "v_w1": v_w1.reshape(6, 12, 1, 1),
            "v_w2": v_w2.reshape(3, 6, 1, 1)}


def test_fixture_is_small_and_seeded():
    fx = golden()
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert fx["features"].shape == (2, 9, 13, 17) and fx["rays"].shape == (2, 6, 13, 17) and fx["v_out"].shape == (2, 3, 13, 17)
    f, r, v = R.seeded_inputs(2, 13, 17)
    assert np.array_equal(f.numpy(), fx["features"]) and np.array_equal(r.numpy(), fx["rays"]) and np.array_equal(v.numpy(), fx["v_out"])
    w1, w2 = R.seeded_weights()
    assert np.array_equal(w1.numpy(), fx["w1"]) and np.array_equal(w2.numpy(), fx["w2"])
    np.testing.assert_allclose(np.linalg.norm(fx["rays"][:, 3:6], axis=1), 1.0, rtol=1e-6)


def test_float64_restatement_reproduces_the_reference():
    fx = golden()
    got = restated(fx)
    e64 = {k: R.rel_l2(v, fx[k + "_f64"]) for k, v in got.items()}
    e32 = {k: R.rel_l2(v, fx[k + "_f32"]) for k, v in got.items()}
    print("\n[restatement vs reference] float64: " + " ".join(f"{k} {v:.2e}" for k, v in e64.items())
          + " | float32: " + " ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    assert all(v <= 1e-12 for v in e64.values()), e64
    assert all(v <= 1e-5 for v in e32.values()), e32


def test_backward_formulas_agree_with_autograd():
    fx = golden()
    T = lambda k: torch.tensor(fx[k], dtype=torch.float64)  # noqa: E731
    f = T("features").permute(0, 2, 3, 1).clone().requires_grad_(True)
    w1, w2 = T("w1").requires_grad_(True), T("w2").requires_grad_(True)
    v = T("v_out").permute(0, 2, 3, 1)
    (R.decode(f, T("rays"), w1, w2) * v).sum().backward()
    v_f, v_w1, v_w2 = R.backward(f.detach(), T("rays"), w1.detach(), w2.detach(), v)
    assert R.rel_l2(v_f, f.grad) <= 1e-12 and R.rel_l2(v_w1, w1.grad.reshape(6, 12)) <= 1e-12
    assert R.rel_l2(v_w2, w2.grad.reshape(3, 6)) <= 1e-12


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 37, 53), (1, 270, 480)])
def test_relu_mask_share_of_the_seeded_inputs(shape):
    """The share of pixels the GPU tests mask (a float64 pre-activation within 1e-5 of zero) stays under 0.1 %."""
    f, r, _ = R.seeded_inputs(*shape)
    w1, _ = R.seeded_weights()
    keep = R.relu_mask(f.permute(0, 2, 3, 1), r, w1)
    share = 1.0 - float(keep.double().mean())
    print(f"\n[relu mask {shape}] masked share {share:.2e}")
    assert share <= R.MASK_SHARE


def test_sandwich_is_the_reference_module_for_a_state_dict():
    from gscodec_studio_amd.dynamic import Sandwich, getcolormodel

    fx = golden()
    m = getcolormodel()
    assert isinstance(m, Sandwich)
    sd = m.state_dict()
    assert list(sd) == ["mlp1.weight", "mlp2.weight"]
    assert sd["mlp1.weight"].shape == fx["w1"].shape == (6, 12, 1, 1) and sd["mlp2.weight"].shape == fx["w2"].shape == (3, 6, 1, 1)
    assert all(v.dtype == torch.float32 for v in sd.values())
    m.load_state_dict({"mlp1.weight": torch.tensor(fx["w1"]), "mlp2.weight": torch.tensor(fx["w2"])}, strict=True)
    assert np.array_equal(m.mlp1.weight.detach().numpy(), fx["w1"]) and np.array_equal(m.mlp2.weight.detach().numpy(), fx["w2"])
    # and the other way: two plain convolutions under the reference's names take this module's state
    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp1 = torch.nn.Conv2d(12, 6, kernel_size=1, bias=False)
            self.mlp2 = torch.nn.Conv2d(6, 3, kernel_size=1, bias=False)

    Plain().load_state_dict(m.state_dict(), strict=True)


@pytest.mark.parametrize("seed", [0, 7])
def test_sandwich_initialises_like_two_convolutions_in_order(seed):
    from gscodec_studio_amd.dynamic import getcolormodel

    torch.manual_seed(seed)
    m = getcolormodel()
    torch.manual_seed(seed)
    a = torch.nn.Conv2d(12, 6, kernel_size=1, bias=False)
    b = torch.nn.Conv2d(6, 3, kernel_size=1, bias=False)
    assert torch.equal(m.mlp1.weight, a.weight) and torch.equal(m.mlp2.weight, b.weight)
    if seed == 0:
        fx = golden()
        assert np.array_equal(m.mlp1.weight.detach().numpy(), fx["w1"]) and np.array_equal(m.mlp2.weight.detach().numpy(), fx["w2"])


def test_refusals():
    from gscodec_studio_amd import dynamic as D

    with pytest.raises(NotImplementedError, match="bias"):
        D.Sandwich(9, 3, bias=True)
    m = D.getcolormodel()
    f, r = torch.zeros(1, 9, 4, 5), torch.zeros(1, 6, 4, 5)
    with pytest.raises(NotImplementedError, match="rays"):
        m(f, r.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(f, r)
    with pytest.raises(RuntimeError, match="no CPU"):
        D.decode_colors(torch.zeros(1, 4, 5, 10), r, m.mlp1.weight, m.mlp2.weight)
    with pytest.raises(ValueError, match=r"\[C, 9, H, W\]"):
        m(torch.zeros(1, 10, 4, 5), r)
    with pytest.raises(ValueError, match="rays must be"):
        m(f, torch.zeros(1, 5, 4, 5))
    with pytest.raises(ValueError, match="float32"):
        m(f.double(), r)
    with pytest.raises(ValueError, match=">= 9"):
        D.decode_colors(torch.zeros(1, 4, 5, 8), r, m.mlp1.weight, m.mlp2.weight)
    with pytest.raises(ValueError, match="w1 must be"):
        D.decode_colors(torch.zeros(1, 4, 5, 9), r, m.mlp2.weight, m.mlp1.weight)
    with pytest.raises(ValueError, match="decoder needs"):
        D.render_dynamic({}, 0.5, None, None, 8, 8, decoder=m)
    with pytest.raises(ValueError, match="decoder needs"):
        D.render_dynamic({}, 0.5, None, None, 8, 8, features="stg", decoder=m)
    x = torch.linspace(-2, 2, 9)
    assert torch.equal(D.trbfunction(x), torch.exp(-1 * x.pow(2)))
    for name in ("Sandwich", "getcolormodel", "decode_colors", "trbfunction"):
        import gscodec_studio_amd

        assert name in gscodec_studio_amd.__doc__, name
    prev = D._set_decoder_tuning(max_blocks=2)
    assert prev == {"max_blocks": 0} and D._set_decoder_tuning(**prev) == {"max_blocks": 2}
    assert D._set_decoder_tuning() == {"max_blocks": 0}


def test_entry_points_are_declared_exported_and_refuse_before_launch():
    from gscodec_studio_amd import _backend as B

    protos = B.prototypes()
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gs_stg_decode_fwd", "gs_stg_decode_bwd", "gs_stg_decode_partial_rows"):
        assert name in protos and name + "(" in hdr, name
        assert hasattr(B.lib(), name), name
    assert B.header_abi_version() == 6
    # fwd: C, H, W, features, pix_stride, rays, cam stride, channel stride, w1, w2, max_blocks, out, stream
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_stg_decode_fwd", 1, 4, 5, None, 9, None, 120, 20, None, None, 0, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):  # no output (fake, never dereferenced, non-null inputs)
        B.call("gs_stg_decode_fwd", 1, 4, 5, 64, 9, 64, 120, 20, 64, 64, 0, None, None)
    with pytest.raises(RuntimeError, match="empty shape"):
        B.call("gs_stg_decode_fwd", 1, 0, 5, 64, 9, 64, 120, 20, 64, 64, 0, 64, None)
    with pytest.raises(RuntimeError, match="pixel stride"):
        B.call("gs_stg_decode_fwd", 1, 4, 5, 64, 8, 64, 120, 20, 64, 64, 0, 64, None)
    with pytest.raises(RuntimeError, match="2\\^32"):
        B.call("gs_stg_decode_fwd", 4, 32768, 32768, 64, 9, 64, 6 << 30, 1 << 30, 64, 64, 0, 64, None)
    with pytest.raises(RuntimeError, match="negative ray strides"):
        B.call("gs_stg_decode_fwd", 1, 4, 5, 64, 9, 64, 120, -20, 64, 64, 0, 64, None)
    with pytest.raises(RuntimeError, match="aligned"):
        B.call("gs_stg_decode_fwd", 1, 4, 5, 66, 9, 64, 120, 20, 64, 64, 0, 64, None)
    # bwd: ..., w2, v_out, max_blocks, v_features, partials, stream
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_stg_decode_bwd", 1, 4, 5, None, 9, None, 120, 20, None, None, None, 0, None, None, None)
    with pytest.raises(RuntimeError, match="no upstream gradient"):
        B.call("gs_stg_decode_bwd", 1, 4, 5, 64, 9, 64, 120, 20, 64, 64, None, 0, 64, 64, None)
    with pytest.raises(RuntimeError, match="no output"):
        B.call("gs_stg_decode_bwd", 1, 4, 5, 64, 9, 64, 120, 20, 64, 64, 64, 0, None, None, None)
    with pytest.raises(RuntimeError, match="pixel stride"):
        B.call("gs_stg_decode_bwd", 1, 4, 5, 64, 3, 64, 120, 20, 64, 64, 64, 0, 64, 64, None)
    with pytest.raises(RuntimeError, match="2\\^32"):
        B.call("gs_stg_decode_bwd", 65536, 256, 256, 64, 9, 64, 6 << 16, 1 << 16, 64, 64, 64, 0, 64, 64, None)
    rows = lambda *a: int(B.query("gs_stg_decode_partial_rows", *a))  # noqa: E731
    assert rows(1, 5, 7, 0) == 1 and rows(2, 37, 53, 2) == 2 and rows(2, 37, 53, 0) == 16
    assert rows(1, 270, 480, 0) == 507 and rows(1, 1080, 1920, 0) == rows(4, 1080, 1920, 0) == 2048
