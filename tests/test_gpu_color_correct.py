"""gscodec_studio_amd.color_correct on the GPU (csrc/color_correct.hip).

The bar: max|ours - float64| <= 4 * E32, where E32 is the largest max|float32 run - float64 run| of the reference's own function
over tests/golden/color_correct.npz (its own float32 error; the factor 4 is the project's convention, as in the surfel tests).
Every fixture case is held to both recorded outputs (the float32 one through the triangle inequality, 5 * E32); fresh larger
cases -- an odd-sized image and the colour columns of a 4-channel render, with the workgroup count forced to 2 (a grid-stride
loop) and at its default (many partial records) -- are held to the numpy restatement of tests/color_correct_reference.py, which
tests/test_color_correct_cpu.py holds to the fixture.  All inputs stay away from the clipping thresholds (asserted), because one
flipped mask bit moves the fit far more than rounding does.  Then: per_image against one call per image, a strided view against
its copy and two runs, all bit for bit; the launch count; degenerate systems; no host synchronisation."""
import functools

import numpy as np
import pytest
import torch

import color_correct_reference as R
from test_color_correct_cpu import CASES, MIN_DISTANCE, e32_max, golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FACTOR = 4
FRESH_SHAPE = (1, 97, 131, 3)  # 12707 pixels: no multiple of the workgroup or of the wave, 13 workgroups by default
FRESH_DISTANCE = 1e-3


def _gpu(a):
    return torch.as_tensor(np.array(a), device=DEV)  # (a copy: the shared references are read-only)


def _err(got, want):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - np.asarray(want, np.float64)).max())


@functools.lru_cache(maxsize=None)
def _fresh():
    """(img, ref, alpha, restatement, threshold distance) of the fresh case: colours inside [0.1, 0.9] and a mild transform."""
    rs = np.random.RandomState(21)
    img = rs.uniform(0.15, 0.85, FRESH_SHAPE)
    mix = np.eye(3) * 0.9 + 0.05 * rs.uniform(-1.0, 1.0, (3, 3))
    ref = np.clip(img @ mix + 0.08 * img * img - 0.01 + 0.01 * rs.standard_normal(FRESH_SHAPE), 0.1, 0.9)
    img, ref = img.astype(np.float32), ref.astype(np.float32)
    alpha = rs.uniform(0.0, 1.0, FRESH_SHAPE[:-1] + (1,)).astype(np.float32)
    want, dist = R.color_correct(img, ref)
    for a in (img, ref, alpha, want):
        a.setflags(write=False)
    return img, ref, alpha, want, dist


@pytest.mark.parametrize("case", CASES)
def test_against_the_reference_fixture(case):
    from gscodec_studio_amd.color_correct import color_correct

    fx = golden()
    bar = FACTOR * e32_max(fx)
    img, ref = _gpu(fx[f"{case}.img"]), _gpu(fx[f"{case}.ref"]).requires_grad_(True)
    out = color_correct(img, ref)
    assert out.shape == img.shape and out.dtype == torch.float32 and not out.requires_grad and out.is_contiguous()
    assert out.data_ptr() != img.data_ptr()
    e64, e32 = _err(out, fx[f"{case}.out64"]), _err(out, fx[f"{case}.out32"])
    print(f"\n[color_correct vs reference, {case}] ours vs float64 {e64:.2e} (bar {bar:.2e}), vs float32 {e32:.2e}; "
          f"the reference's float32 vs float64 {float(fx[f'{case}.e32']):.2e}")
    assert float(fx[f"{case}.distance"]) >= MIN_DISTANCE
    assert e64 <= bar
    assert e32 <= bar + e32_max(fx)


@pytest.mark.parametrize("workgroups", [2, None], ids=["two_workgroups", "default"])
@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "render_view"])
def test_fresh_image_against_the_restatement(view, workgroups):
    from gscodec_studio_amd.color_correct import color_correct

    img, ref, alpha, want, dist = _fresh()
    assert dist >= FRESH_DISTANCE
    bar = FACTOR * e32_max()
    x = _gpu(np.concatenate([img, alpha], -1))[..., 0:3] if view else _gpu(img)
    assert x.is_contiguous() != view
    out = color_correct(x, _gpu(ref), workgroups=workgroups)
    err = _err(out, want)
    print(f"\n[color_correct vs restatement, {'render view' if view else 'contiguous'}, workgroups {workgroups}] {err:.2e} "
          f"(bar {bar:.2e}, threshold distance {dist:.2e})")
    assert out.is_contiguous() and err <= bar
    if view:  # read in place through the pixel stride: the same bits as from a copy
        assert torch.equal(out, color_correct(x.contiguous(), _gpu(ref), workgroups=workgroups))


def test_per_image_equals_one_call_per_image_bit_for_bit():
    from gscodec_studio_amd.color_correct import color_correct

    fx = golden()
    img, ref = _gpu(fx["pair_n3.img"]), _gpu(fx["pair_n3.ref"])
    for wg in (None, 3):
        both = color_correct(img, ref, per_image=True, workgroups=wg)
        for i in range(img.shape[0]):
            assert torch.equal(both[i], color_correct(img[i], ref[i], workgroups=wg)), (wg, i)
        assert not torch.equal(both, color_correct(img, ref, workgroups=wg))  # one system for all is another fit
    want, dist = R.color_correct(fx["pair_n3.img"], fx["pair_n3.ref"], per_image=True)
    assert dist >= MIN_DISTANCE and _err(both, want) <= FACTOR * e32_max(fx)
    # the same for a strided batch
    wide = torch.cat([img, torch.rand_like(img[..., :1])], -1)
    assert torch.equal(color_correct(wide[..., 0:3], ref, per_image=True, workgroups=3), both)


def test_two_runs_are_bit_identical():
    from gscodec_studio_amd.color_correct import color_correct

    img, ref, _, _, _ = _fresh()
    x, y = _gpu(img), _gpu(ref)
    assert torch.equal(color_correct(x, y), color_correct(x, y))
    assert torch.equal(color_correct(x, y, workgroups=7), color_correct(x, y, workgroups=7))


def test_num_iters_and_launch_count(monkeypatch):
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.color_correct import color_correct

    fx = golden()
    img, ref = _gpu(fx["image_n3.img"]), _gpu(fx["image_n3.ref"])
    wide = torch.cat([img, img[..., :1]], -1)
    for x in (img, wide[..., 0:3]):
        out = color_correct(x, ref, num_iters=0)
        assert torch.equal(out, img) and out.data_ptr() != x.data_ptr() and out.is_contiguous()
    calls, real = [], B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for iters in (0, 1, 2, 5):
        del calls[:]
        out = color_correct(img, ref, num_iters=iters)
        want = ["gs_color_correct_pass", "gs_color_correct_solve"] * iters + ["gs_color_correct_pass"] * (iters > 0)
        assert calls == want, (iters, calls)
        assert len(calls) == (2 * iters + 1 if iters else 0)
        assert _err(out, R.color_correct(fx["image_n3.img"], fx["image_n3.ref"], num_iters=iters)[0]) <= FACTOR * e32_max(fx)


def _degenerate():
    rs = np.random.RandomState(3)
    ref = rs.uniform(0.1, 0.9, (40, 3)).astype(np.float32)
    const = np.broadcast_to(np.array([0.3, 0.5, 0.7], np.float32), (40, 3)).copy()
    one = rs.uniform(0.1, 0.9, (40, 3)).astype(np.float32)
    one[:, 1] = 1.0
    few = rs.uniform(0.1, 0.9, (5, 3)).astype(np.float32)
    black = np.zeros((40, 3), np.float32)  # every mask empty: every system is the zero matrix
    return {"constant_image": (const, ref), "channel_of_ones": (one, ref), "five_pixels": (few, ref[:5]), "no_rows": (black, ref)}


@pytest.mark.parametrize("name", ["constant_image", "channel_of_ones", "five_pixels", "no_rows"])
def test_degenerate_systems_are_finite_and_minimum_norm(name):
    from gscodec_studio_amd.color_correct import color_correct

    img, ref = _degenerate()[name]
    want, _ = R.color_correct(img, ref)
    out = color_correct(_gpu(img), _gpu(ref))
    assert bool(torch.isfinite(out).all())
    err = _err(out, want)
    print(f"\n[color_correct, {name}] ours vs restatement {err:.2e}")
    assert err <= 1e-6


def test_color_correct_does_not_synchronise():
    from gscodec_studio_amd.color_correct import color_correct

    img, ref, alpha, _, _ = _fresh()
    x, y = _gpu(np.concatenate([img, alpha], -1))[..., 0:3], _gpu(ref)
    first = color_correct(x, y)  # first call: allocations outside the checked window
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = color_correct(x, y, per_image=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second)
