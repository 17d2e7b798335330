"""The hash-grid Gaussian route of the entropy coder on the GPU (csrc/gauss_ans.hip behind gscodec_studio_amd.compression.gauss_ans)
and through EntropyCodingCompression: byte identity with the numpy coder that defines the format, the params kernel against the
stated float32 order element for element, and the directory level with the reference's file names and meta keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gauss_ans_cases import model_case
from util import N, T, golden, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODINGS = ("encoding_xyz", "encoding_xy", "encoding_xz", "encoding_yz")


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("stream_len", [1, 5, 1024])
def test_byte_identity_with_the_numpy_coder(stream_len, channels):
    """N = 1, 7, 1023, 1024, 1025, 3000: one lane, a full and a ragged stream, and (S = 1 and 5: 3000 and 600 streams per channel)
    many workgroups of both kernels.  Either side's stream decodes exactly with the other side's decoder."""
    from gscodec_studio_amd.compression import gauss_ans as GA, gauss_ans_reference as R

    S = stream_len
    for n in (1, 7, 1023, 1024, 1025, 3000):
        sym, mu_q, k = model_case(n, channels, 1000 * n + 10 * channels + S)
        d_mu, d_k = T(mu_q), T(k)
        ours = GA.gauss_ans_encode(T(sym), d_mu, d_k, stream_len=S)
        want = R.encode(sym, mu_q, k, stream_len=S)
        assert ours.dtype == np.uint8 and ours.shape == want.shape and np.array_equal(ours, want), (S, channels, n)
        back = GA.gauss_ans_decode(want, d_mu, d_k, device="cuda")
        assert back.dtype == torch.uint8 and tuple(back.shape) == sym.shape and np.array_equal(N(back), sym), (S, channels, n)


def test_wrong_model_and_refusals():
    from gscodec_studio_amd.compression import gauss_ans as GA, gauss_ans_reference as R

    n = 2048 + 17
    sym = np.random.default_rng(1).integers(0, 40, (n, 2)).astype(np.uint8)
    wrong_mu, k0 = np.full((n, 2), R.MU_Q_MAX, np.int16), np.zeros((n, 2), np.uint8)  # frequency 1 for every symbol: the slot's worst case
    blob = GA.gauss_ans_encode(T(sym), T(wrong_mu), T(k0))
    assert np.array_equal(blob, R.encode(sym, wrong_mu, k0)) and np.array_equal(N(GA.gauss_ans_decode(blob, T(wrong_mu), T(k0))), sym)
    with pytest.raises(RuntimeError):  # CPU tensors
        GA.gauss_ans_encode(torch.from_numpy(sym), T(wrong_mu), T(k0))
    with pytest.raises(RuntimeError):
        GA.gauss_ans_encode(T(sym), torch.from_numpy(wrong_mu), torch.from_numpy(k0))
    with pytest.raises(RuntimeError):
        GA.gauss_ans_decode(blob, T(wrong_mu), T(k0), device="cpu")
    for bad_mu, bad_k in ((wrong_mu + 1, k0), (wrong_mu - 2041, k0), (wrong_mu, k0 + 64), (wrong_mu[:-1], k0[:-1]), (wrong_mu.astype(np.int32), k0)):
        with pytest.raises(ValueError):
            GA.gauss_ans_encode(T(sym), T(bad_mu), T(bad_k))
        with pytest.raises(ValueError):
            GA.gauss_ans_decode(blob, T(bad_mu), T(bad_k))
    with pytest.raises(ValueError, match="not interchangeable"):
        GA.gauss_ans_decode(np.random.default_rng(0).integers(0, 2**32, 500, dtype=np.uint32), T(wrong_mu), T(k0))
    with pytest.raises(ValueError):  # cut short: refused on the host
        GA.gauss_ans_decode(blob[:-100], T(wrong_mu), T(k0))


def test_damaged_and_truncated_payload_stay_in_bounds():
    """A valid container with damaged bytes decodes like the numpy decoder (0 beyond each stream's range).  The kernel handed
    fewer payload bytes than the offsets describe clamps every stream's range to what it was given: the same symbols as the numpy
    decoder on a payload whose missing tail reads as 0."""
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.compression import gauss_ans as GA, gauss_ans_reference as R

    sym, mu_q, k = model_case(70 * 64 + 9, 2, 3)
    blob = R.encode(sym, mu_q, k, stream_len=64)
    bad = blob.copy()
    bad[-3000:] = np.random.default_rng(1).integers(0, 256, 3000, dtype=np.uint8)
    out = N(GA.gauss_ans_decode(bad, T(mu_q), T(k)))
    assert np.array_equal(out, R.decode(bad, mu_q, k)) and not np.array_equal(out, sym)

    c, s_len, n, offsets, payload = R.parse_container(blob)
    keep = payload.size - 2500  # ends inside a stream
    zeroed = blob.copy()
    zeroed[-2500:] = 0
    d_payload, d_off = T(np.array(payload[:keep])), T(offsets)
    d_mu, d_k = T(np.ascontiguousarray(mu_q.T)), T(np.ascontiguousarray(k.T))
    table = T(R.gaussian_table().view(np.int16).copy())
    got = torch.full((n, c), 7, dtype=torch.uint8, device="cuda")
    B.call("gs_gauss_ans_decode", n, c, s_len, B.ptr(d_payload), keep, B.ptr(d_off), B.ptr(d_mu), B.ptr(d_k), B.ptr(table), B.ptr(got),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(N(got), R.decode(zeroed, mu_q, k))


def _model(channel, seed):
    """An Entropy_gaussian in the reference configuration with tables of mixed signs and an MLP whose scale outputs are positive for
    most splats in every channel but the first (the default initialisation leaves about half of them below the 1e-9 clamp)."""
    from gscodec_studio_amd.compression_simulation import Entropy_gaussian

    torch.manual_seed(seed)
    m = Entropy_gaussian(channel=channel)
    with torch.no_grad():
        m.param_regressor.mlp_regressor[2].bias[channel + 1:] += 0.4
    return m.cuda()


def _positions(n, seed):
    """Garden means spread over the model's [-100, 100] box; a few rows outside it (zero features) when n allows."""
    g = torch.Generator().manual_seed(seed)
    fx = torch.from_numpy(golden("garden_small.npz")["means"][:max(n, 8)]).float()
    pos = (fx * 12.0 + torch.randn(fx.shape, generator=g))[:n].clone()
    if n > 8:
        pos[3, 0], pos[5, 2] = 150.0, -101.0
    return pos.cuda()


@pytest.mark.parametrize("channel", [3, 4])
def test_params_kernel_equals_the_stated_order(channel):
    from gscodec_studio_amd.compression import gauss_ans as GA, gauss_ans_reference as R

    m = _model(channel, 10 + channel)
    pr = m.param_regressor
    w = [N(t).astype(np.float32) for t in (pr.mlp_regressor[0].weight, pr.mlp_regressor[0].bias, pr.mlp_regressor[2].weight, pr.mlp_regressor[2].bias)]
    mins = np.array([-0.3, -1.0, 0.1, -2.0][:channel], np.float32)
    maxs = np.array([0.9, 0.5, 0.1 + 2.0 ** -6, 3.0][:channel], np.float32)  # a narrow channel: sigma_norm reaches the upper levels
    for n in (1, 63, 64, 65, 2000):
        pos = _positions(n, n)
        with torch.no_grad():
            feat = pr.hash_grid((pos - pr.bound_min) / (pr.bound_max - pr.bound_min))
        assert tuple(feat.shape) == (n, 48)
        want_mu, want_k, want_miu, want_sigma = R.regress_params(N(feat), *w, mins, maxs, return_float=True)
        mu_q, k, miu, sigma = GA.gaussian_params(m, pos, mins, maxs, return_float=True)
        assert mu_q.dtype == torch.int16 and k.dtype == torch.uint8 and tuple(mu_q.shape) == (n, channel) == tuple(k.shape)
        assert np.array_equal(N(miu).view(np.uint32), want_miu.view(np.uint32)), n  # the float32 order itself
        assert np.array_equal(N(sigma).view(np.uint32), want_sigma.view(np.uint32)), n
        assert np.array_equal(N(mu_q), want_mu) and np.array_equal(N(k), want_k), n
        with torch.no_grad():
            ref_mean, ref_scale = m.get_means_and_scales(pos)  # the module's own GEMMs: another summation order
        for got, ref in ((miu, ref_mean), (sigma, ref_scale)):
            assert rel_l2(N(got), N(ref)) <= 1e-5 and float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        if n == 2000:
            assert len(np.unique(want_k)) > 8 and 0 < (want_mu == 0).mean() < 0.9 and (want_sigma == np.float32(1e-9)).any()
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:777].cuda()
            sub_mu, sub_k = GA.gaussian_params(m, pos[perm], mins, maxs)  # a splat's model depends on its position alone
            assert torch.equal(sub_mu, mu_q[perm]) and torch.equal(sub_k, k[perm])


def test_params_refusals():
    from gscodec_studio_amd.compression import gauss_ans as GA
    from gscodec_studio_amd.compression_simulation import Entropy_factorized_optimized_refactor, Entropy_gaussian

    pos = _positions(100, 0)
    m = _model(3, 0)
    with pytest.raises(RuntimeError):
        GA.gaussian_params(m, pos.cpu(), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError):
        GA.gaussian_params(m, pos, [0, 0], [1, 1])
    with pytest.raises(ValueError):
        GA.gaussian_params(Entropy_gaussian(channel=9).cuda(), pos, [0] * 9, [1] * 9)
    with pytest.raises(ValueError):
        GA.gaussian_params(Entropy_factorized_optimized_refactor(channel=3).cuda(), pos, [0, 0, 0], [1, 1, 1])
    wide = Entropy_gaussian(channel=3).cuda()
    wide.param_regressor.mlp_regressor[0] = torch.nn.Linear(48, 16).cuda()
    with pytest.raises(ValueError):
        GA.gaussian_params(wide, pos, [0, 0, 0], [1, 1, 1])
    plain = _model(3, 1)
    plain.param_regressor.hash_grid.encoding_xz.ste_binary = False
    with pytest.raises(ValueError):
        GA.gaussian_params(plain, pos, [0, 0, 0], [1, 1, 1])
    with torch.no_grad():
        m.param_regressor.hash_grid.encoding_xy.params[5, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        GA.gaussian_params(m, pos, [0, 0, 0], [1, 1, 1])


def _splats(n=2500):
    """The 2,500-splat crop of the garden fixture of test_gpu_ans.py: seeded raw attributes, every 50th splat transparent, so that
    the opacity filter and the crop to a square count both drop splats (-> 49^2)."""
    fx = golden("garden_small.npz")
    g = torch.Generator().manual_seed(9)
    shN = torch.randn(n, 3, 3, generator=g) * 0.1
    shN[::4] = -shN[::4].abs()
    opacities = torch.randn(n, generator=g) * 2 + 1
    opacities[::50] = -8.0
    s = {"means": torch.from_numpy(fx["means"][:n]), "scales": torch.log(torch.from_numpy(fx["scales"][:n]) + 1e-4),
         "quats": torch.from_numpy(fx["quats"][:n]) * (0.5 + torch.rand(n, 1, generator=g)),
         "opacities": opacities, "sh0": torch.randn(n, 1, 3, generator=g), "shN": shN}
    return {k: v.float().cuda() for k, v in s.items()}


_CHILD = """
import sys
import numpy as np
from gscodec_studio_amd.compression import EntropyCodingCompression
reg = {a: {"encode": "_compress_gaussian_ans", "decode": "_decompress_gaussian_ans"} for a in ("scales", "quats")}
out = EntropyCodingCompression(attribute_codec_registry=reg).decompress(sys.argv[1])
np.savez(sys.argv[2], **{k: v.cpu().numpy() for k, v in out.items()})
"""


def test_directory_round_trip(tmp_path):
    from gscodec_studio_amd.compression import EntropyCodingCompression, dequantize_grid, quantize_grid
    from gscodec_studio_amd.compression import gauss_ans_reference as R
    from gscodec_studio_amd.compression._container import prepare_splats
    from gscodec_studio_amd.compression_simulation import Entropy_gaussian, HashGridCompressionSimulation, STE_binary

    splats = _splats()
    steps = {"means": -1, "scales": 10, "quats": 20, "opacities": -1, "sh0": 30, "shN": -1}
    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda")
    params = {k: torch.nn.Parameter(v.clone()) for k, v in splats.items()}
    with torch.no_grad():
        sim._estiblish_bbox(params["means"])
    torch.manual_seed(3)
    for _ in range(3):  # a few optimizer steps: the tables leave their +-1e-4 initialisation, the MLP moves
        _, bits = sim.simulate_compression(params, step=35)
        sum(b.sum() / b.numel() for b in bits.values() if b is not None).backward()
        for a in ("scales", "quats"):
            sim.entropy_model_optimizers[a].step()
            sim.entropy_model_optimizers[a].zero_grad()
    for a in ("scales", "quats"):
        for e in ENCODINGS:  # (where the rate term's gradient vanishes the tables keep their initial signs, which are mixed too)
            t = getattr(sim.entropy_models[a].param_regressor.hash_grid, e).params.detach()
            assert 0.05 < float((t >= 0).float().mean()) < 0.95, (a, e)

    reg = {a: {"encode": "_compress_gaussian_ans", "decode": "_decompress_gaussian_ans"} for a in ("scales", "quats")}
    d, d0 = str(tmp_path / "gauss"), str(tmp_path / "factorized")
    before = {k: v.clone() for k, v in splats.items()}
    codec = EntropyCodingCompression(use_sort="morton", verbose=False, n_clusters=256, attribute_codec_registry=reg)
    codec.compress(d, splats, entropy_models=sim.entropy_models)
    assert all(torch.equal(splats[k], before[k]) for k in before)
    names = "means_l.png means_u.png scales.bin quats.bin opacities.png sh0.png shN.npz mask.bin meta.json".split()
    names += [f"{a}_entropy_model_{e}.bin" for a in ("scales", "quats") for e in ENCODINGS]
    names += [f"{a}_entropy_model_mlp.ckpt" for a in ("scales", "quats")]
    assert sorted(os.listdir(d)) == sorted(names)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    assert list(meta) == ["means", "scales", "quats", "opacities", "sh0", "shN"]
    for a in ("scales", "quats"):
        assert set(meta[a]) == {"shape", "dtype", "mins", "maxs"} | {f"{e}_shape" for e in ENCODINGS}, a
        pr = sim.entropy_models[a].param_regressor
        for e in ENCODINGS:
            table = getattr(pr.hash_grid, e).params
            assert meta[a][f"{e}_shape"] == list(table.shape)
            data = np.fromfile(os.path.join(d, f"{a}_entropy_model_{e}.bin"), np.uint8)
            signs = N(STE_binary.apply(table.detach())).reshape(-1)
            assert data.size == (signs.size + 7) // 8 and np.array_equal(R.unpack_signs(data, signs.size), signs)
        fresh = Entropy_gaussian(channel=meta[a]["shape"][-1])
        state = torch.load(os.path.join(d, f"{a}_entropy_model_mlp.ckpt"), map_location="cpu")
        fresh.param_regressor.mlp_regressor.load_state_dict(state, strict=True)
        for key, v in pr.mlp_regressor.state_dict().items():
            assert torch.equal(state[key], v.cpu()), key
        assert open(os.path.join(d, f"{a}.bin"), "rb").read(8) == b"GSGANSv1"
    out = codec.decompress(d)

    kept, side = prepare_splats(splats, 0.005, "morton", False)
    assert side == 49
    for a in ("scales", "quats"):  # the dequantised direct 8-bit symbols, bit for bit
        (plane,), m = quantize_grid(kept[a], side, bits=8)
        assert torch.equal(out[a], dequantize_grid([plane.reshape(side * side, -1)], m)), a

    # the factorized directory of the same splats: every other file and every decoded tensor is the same
    plain = EntropyCodingCompression(use_sort="morton", verbose=False, n_clusters=256)
    plain.compress(d0, splats, entropy_models=sim.entropy_models)
    for name in "means_l.png means_u.png opacities.png sh0.png mask.bin".split():
        assert open(os.path.join(d, name), "rb").read() == open(os.path.join(d0, name), "rb").read(), name
    want = plain.decompress(d0)
    assert set(out) == set(want) and all(torch.equal(out[k], want[k]) for k in want)
    sizes = {a: (os.path.getsize(os.path.join(d, f"{a}.bin")), os.path.getsize(os.path.join(d0, f"{a}.bin"))) for a in ("scales", "quats")}
    print(f"bytes of <name>.bin after 3 optimizer steps of the model (Gaussian route, factorized route): {sizes}")

    # a fresh codec in a fresh process reads the same directory to the same tensors
    npz = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, d, npz], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = np.load(npz)
    assert set(child.files) == set(out)
    for k in out:
        assert np.array_equal(child[k].view(np.uint32), N(out[k]).view(np.uint32)), k

    # the two misuses keep their error
    with pytest.raises(NotImplementedError, match="hash-grid Gaussian"):
        codec.compress(str(tmp_path / "none"), splats, entropy_models={"scales": sim.entropy_models["scales"]})
    with pytest.raises(NotImplementedError, match="hash-grid Gaussian"):
        codec.decompress(d0)
