"""The appearance module without a GPU (gscodec_studio_amd.appearance.AppearanceOptModule): the module's parameters against
tests/golden/appearance.npz (the reference class's seeded state), checkpoint loading both ways, the float64 restatement of
tests/appearance_reference.py against the reference class's own float32 results, and every refusal that comes before a launch."""
import functools
import os

import numpy as np
import pytest
import torch

import appearance_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "appearance.npz")
DEGREES = (0, 2, 3)
PARAMS = ("embeds.weight",) + R.STATE_KEYS


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_state():
    return {k: torch.from_numpy(golden()["state." + k]) for k in PARAMS}


def _module(*a, **kw):
    from gscodec_studio_amd.appearance import AppearanceOptModule

    return AppearanceOptModule(*a, **kw)


def test_state_dict_matches_the_reference_seeded_state():
    torch.manual_seed(0)
    m = _module(5, 32)
    sd = m.state_dict()
    assert tuple(sd) == PARAMS
    for k, want in golden_state().items():
        assert sd[k].shape == want.shape and sd[k].dtype == torch.float32, k
        assert torch.equal(sd[k], want), k


def test_strict_loading_both_ways():
    m = _module(5, 32)
    m.load_state_dict(golden_state(), strict=True)
    for k, want in golden_state().items():
        assert torch.equal(m.state_dict()[k], want)
    # the reference's layout, built from plain torch layers in its order
    other = torch.nn.Module()
    other.embeds = torch.nn.Embedding(5, 16)
    other.color_head = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 64),
                                           torch.nn.ReLU(inplace=True), torch.nn.Linear(64, 3))
    other.load_state_dict(m.state_dict(), strict=True)
    # the trainer's initialisation of the last layer keeps working
    torch.nn.init.zeros_(m.color_head[-1].weight)
    assert float(m.color_head[4].weight.detach().abs().sum()) == 0.0


@pytest.mark.parametrize("deg", DEGREES)
def test_restatement_reproduces_the_reference(deg):
    """float64 restatement vs the reference class's float32 results: 2e-6 relative L2 (the reference's own float32-vs-float64
    differences are 4e-8 to 4e-7)."""
    g = golden()
    P = {k: t.requires_grad_(True) for k, t in R.head_of(golden_state()).items()}
    emb_w = golden_state()["embeds.weight"].double().requires_grad_(True)
    f, d, b = (torch.from_numpy(g[k]).double().requires_grad_(True) for k in ("features", "dirs", "base"))
    ids = torch.from_numpy(g["ids"])
    raw = R.forward(P, f, emb_w[ids], d, 16, deg)
    out = torch.sigmoid(raw + b[None])
    (out * torch.from_numpy(g["v_out"]).double()).sum().backward()
    got = {"raw": raw, "out": out, "v_features": f.grad, "v_base": b.grad, "v_embeds.weight": emb_w.grad,
           "v_dirs": d.grad if d.grad is not None else torch.zeros_like(d)}
    got.update({"v_" + s: P[k].grad for k, s in zip(R.HEAD, R.STATE_KEYS)})
    for k, t in got.items():
        want = g[f"{k}_d{deg}"]
        err = R.rel_l2(t.detach(), want)
        print(f"[deg {deg}] {k}: {err:.2e}")
        assert err < 2e-6, (k, err)
    # bases above the degree in use: zero columns of the first layer's gradient
    nb = (deg + 1) ** 2
    assert float(P["w1"].grad[:, 48 + nb:].abs().max() if nb < 16 else 0.0) == 0.0
    assert float(np.abs(g[f"v_color_head.0.weight_d{deg}"][:, 48 + nb:]).max() if nb < 16 else 0.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_sizes_are_refused():
    for kw in (dict(mlp_width=32), dict(mlp_depth=3), dict(mlp_depth=1), dict(sh_degree=5)):
        with pytest.raises(NotImplementedError):
            _module(4, 32, **kw)
    with pytest.raises(NotImplementedError):
        _module(4, 100, embed_dim=16, sh_degree=3)  # 132 inputs
    with pytest.raises(NotImplementedError):
        _module(4, 97, embed_dim=0, sh_degree=0)  # more than three feature tiles
    _module(4, 32, embed_dim=0)
    _module(4, 32, embed_dim=16, sh_degree=4)  # 73 inputs: the padded path


def _args(N=7, C=2):
    return torch.zeros(N, 32), torch.tensor([0, 1][:C]), torch.ones(C, N, 3)


def test_cpu_tensors_are_refused():
    m = _module(4, 32)
    f, ids, d = _args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(f, ids, d, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.colors(f, ids, torch.zeros(7, 3), torch.eye(4).expand(2, 4, 4), 3, base=torch.zeros(7, 3))


def test_wrong_dtypes_and_shapes_are_refused():
    m = _module(4, 32)
    f, ids, d = _args()
    with pytest.raises(ValueError, match="float32"):
        m(f.double(), ids, d, 3)
    with pytest.raises(ValueError, match="float32"):
        m(f, ids, d.half(), 3)
    with pytest.raises(ValueError, match="features"):
        m(torch.zeros(7, 31), ids, d, 3)
    with pytest.raises(ValueError, match="dirs"):
        m(f, ids, torch.ones(2, 8, 3), 3)
    with pytest.raises(ValueError, match="sh_degree"):
        m(f, ids, d, 4)
    eye = torch.eye(4).expand(2, 4, 4)
    with pytest.raises(ValueError, match="means"):
        m.colors(f, ids, torch.zeros(8, 3), eye, 3)
    with pytest.raises(ValueError, match="camtoworlds"):
        m.colors(f, ids, torch.zeros(7, 3), torch.eye(4), 3)
    with pytest.raises(ValueError, match="base"):
        m.colors(f, ids, torch.zeros(7, 3), eye, 3, base=torch.zeros(7, 4))
    with pytest.raises(ValueError, match="float32"):
        m.colors(f, ids, torch.zeros(7, 3), eye.double(), 3)
    with pytest.raises(NotImplementedError, match="drop-in form"):
        m.colors(f, ids, torch.zeros(7, 3), eye.clone().requires_grad_(True), 3)
    # a head that no longer has the kernels' shapes
    m.color_head[4] = torch.nn.Linear(64, 4)
    with pytest.raises(NotImplementedError):
        m(f, ids, d, 3)
