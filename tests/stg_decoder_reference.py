"""The spacetime colour decoder restated in torch, written from its formulas (any dtype; the tests use float64).

Per pixel, with f[0..8] the rendered feature and r[0..5] the ray:
    x[0..11] = (f[3..8], r[0..5])
    h[j]     = max(0, sum_k W1[j][k] x[k])            j = 0..5
    out[c]   = sigmoid(f[c] + sum_j W2[c][j] h[j])    c = 0..2
Features are NHWC [C, H, W, 9], rays [C, 6, H, W], W1 [6, 12] and W2 [3, 6] (trailing 1x1 dimensions are dropped)."""
import numpy as np
import torch

MASK_EPS = 1e-5      # a float64 pre-activation of h closer to zero than this: the pixel's ReLU decision may flip in float32
MASK_SHARE = 1e-3    # at most 0.1 % of the pixels may be masked


def pre_activation(features, rays, w1):
    """[C, H, W, 6]: sum_k W1[j][k] x[k]."""
    x = torch.cat((features[..., 3:9], rays.permute(0, 2, 3, 1)), dim=-1)
    return x @ w1.reshape(6, 12).T, x


def decode(features, rays, w1, w2):
    """[C, H, W, 3]."""
    pre, _ = pre_activation(features, rays, w1)
    h = torch.clamp_min(pre, 0)
    return torch.sigmoid(features[..., 0:3] + h @ w2.reshape(3, 6).T)


def backward(features, rays, w1, w2, v_out):
    """(v_features [C, H, W, 9], v_w1 [6, 12], v_w2 [3, 6]) from the formulas, no autograd."""
    pre, x = pre_activation(features, rays, w1)
    h = torch.clamp_min(pre, 0)
    w2m = w2.reshape(3, 6)
    out = torch.sigmoid(features[..., 0:3] + h @ w2m.T)
    g = v_out * out * (1 - out)
    v_h = (g @ w2m) * (h > 0).to(g.dtype)
    v_f = torch.cat((g, v_h @ w1.reshape(6, 12)[:, 0:6]), dim=-1)
    v_w2 = g.reshape(-1, 3).T @ h.reshape(-1, 6)
    v_w1 = v_h.reshape(-1, 6).T @ x.reshape(-1, 12)
    return v_f, v_w1, v_w2


def relu_mask(features, rays, w1):
    """bool [C, H, W, 1]: pixels to KEEP (no float64 pre-activation of h within MASK_EPS of zero)."""
    pre, _ = pre_activation(features.double(), rays.double(), w1.double())
    return (pre.abs() >= MASK_EPS).all(dim=-1, keepdim=True)


def seeded_weights():
    """(w1 [6, 12, 1, 1], w2 [3, 6, 1, 1]): two 1x1 convolutions created in the module's order under torch.manual_seed(0)."""
    torch.manual_seed(0)
    a = torch.nn.Conv2d(12, 6, kernel_size=1, bias=False)
    b = torch.nn.Conv2d(6, 3, kernel_size=1, bias=False)
    return a.weight.detach().clone(), b.weight.detach().clone()


def seeded_inputs(C, H, W, seed=1):
    """(features NCHW [C, 9, H, W], rays [C, 6, H, W] with unit directions, v_out NCHW [C, 3, H, W]): standard normal, float32, CPU."""
    g = torch.Generator().manual_seed(seed)
    features = torch.randn((C, 9, H, W), generator=g)
    rays = torch.randn((C, 6, H, W), generator=g)
    v_out = torch.randn((C, 3, H, W), generator=g)
    rays[:, 3:6] = rays[:, 3:6] / rays[:, 3:6].norm(dim=1, keepdim=True)
    return features, rays, v_out


def rel_l2(got, want):
    want = torch.as_tensor(np.asarray(want) if not isinstance(want, torch.Tensor) else want).double().cpu()
    got = torch.as_tensor(np.asarray(got) if not isinstance(got, torch.Tensor) else got).double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))
