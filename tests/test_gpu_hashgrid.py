"""GPU: the hash-grid Gaussian entropy model (csrc/hashgrid.hip) against the float64 restatement of
tests/hashgrid_reference.py -- encoder forward / table gradient / reference-formula input gradient through the C ABI with
guard bands, exactness on dyadic inputs, STE values and mask, determinism, rejections, the modules
(GridEncoder, mix_3D2D_encoding, Entropy_gaussian) and HashGridCompressionSimulation, and the Gaussian bits kernels.

Bars.  Encoder forward, table gradient, input gradient: 1e-4 relative L2 per tensor (the project's bar); the input gradient
jumps at cell faces, so points closer than 1e-5 (in cells) to a face at any level are left out (at most 1 %, asserted on the
restatement).  Bits: |err| <= 1e-4 |bits| + 4e-3 where the float64 likelihood is >= 1e-4 (the bar of test_gpu_entropy.py);
below 1e-4 the kernel's worst error may not exceed the worst error of the float32 torch form on the same inputs plus the
4e-3 floor; gradients within 1e-4 of the tensor's scale, elements within 2e-7 of the bound left out (at most 1 %).
Every comparison prints its figure and its share of the bar ("[hashgrid] ...").

Measured on an MI355X with this file (profiles/r24_hashgrid.txt), worst of each kind: encoder forward 4.7e-8, table gradient
3.1e-7, input gradient 7.0e-8 (bar 1e-4), table gradient run to run 2.0e-7 (bar 1e-5); Entropy_gaussian(3) / (4): bits 0.4 % of
the bar, gradients 3.4e-6; bits kernel: 0.3 % of the bar above a likelihood of 1e-4, 1.8e-5 bits below it (float32 torch
form: 0.10 bits), gradients 1.7e-6 of the tensor's scale.
"""
import copy
import functools
import math

import pytest
import torch

import hashgrid_reference as HR
from test_hashgrid_cpu import BAD_ENCODE, BAD_ENCODE_BWD, BAD_ENCODE_FWD, ENC_BASE, abi_encode, bits_inputs, small_grids
from util import garden

pytestmark = pytest.mark.gpu

BAR = 1e-4
BOUND = 1e-6
GUARD = 4096           # floats on each side of a buffer the kernels write
SENTINEL = 0x7FC0BEEF  # a NaN bit pattern no kernel produces
AXES_CODE = {(0, 1, 2): 0, (0, 1): 1, (0, 2): 2, (1, 2): 3}
AXES_OF = {"xyz": (0, 1, 2), "xy": (0, 1), "xz": (0, 2), "yz": (1, 2)}
NAN = float("nan")
# exact 0, exact 1, 0.5, a coordinate just below 0 / just above 1 / NaN (x, and z), cells that touch the border
SPECIAL = [[0, 0, 0], [1, 1, 1], [.5, .5, .5], [-1e-3, .3, .4], [.2, 1.001, .6], [NAN, .3, .7], [.3, .4, NAN], [.01, .5, .5],
           [.99, .02, .5], [.5, .5, .995]]
BAD_AXIS = {3: 0, 4: 1, 5: 0, 6: 2}  # row of SPECIAL -> its out-of-range column


def report(label, value, bar):
    print(f"[hashgrid] {label}: {value:.3e} / bar {bar:.1e} = {value / bar:.3f}")
    return value


def rel_l2(a, e):
    a, e = a.detach().double(), e.detach().double()
    return float((a - e).norm() / max(float(e.norm()), 1e-30))


def guarded(numel, fill=None):
    whole = torch.empty(numel + 2 * GUARD, dtype=torch.float32, device="cuda")
    whole.view(torch.int32).fill_(SENTINEL)
    inner = whole[GUARD:GUARD + numel]
    if fill is not None:
        inner.fill_(fill)
    return whole, inner


def guards_intact(whole, numel):
    torch.cuda.synchronize()
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + numel:] == SENTINEL).all())


def untouched(whole):
    torch.cuda.synchronize()
    return bool((whole.view(torch.int32) == SENTINEL).all())


def positions(n, seed=1):
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed))
    k = min(n, len(SPECIAL))
    pos[:k] = torch.tensor(SPECIAL[:k])
    return pos


def abi_args(pos_t, grids, tables, ste):
    return dict(n=pos_t.shape[0], pos_dim=pos_t.shape[1], n_grids=len(grids), F=tables[0].shape[1], ste=int(ste), pos=pos_t.data_ptr(),
                params=[t.data_ptr() for t in tables], rows=[t.shape[0] for t in tables], num_dim=[g["num_dim"] for g in grids],
                axes=[AXES_CODE[tuple(g["axes"])] for g in grids], n_levels=[len(g["resolutions"]) for g in grids],
                res=[r for g in grids for r in g["resolutions"]], off=[o for g in grids for o in g["offsets"]])


def width(grids):
    return sum(len(g["resolutions"]) for g in grids) * grids[0]["params"].shape[1]


def run_abi(pos, grids, ste, v_out, stream=None):
    """Forward and backward through the C ABI with guard bands -> (out, [v_params], v_pos) on the CPU."""
    n, W = pos.shape[0], width(grids)
    pos_t, tables = pos.cuda(), [g["params"].float().cuda() for g in grids]
    a = abi_args(pos_t, grids, tables, ste)
    out_w, out = guarded(n * W)
    abi_encode(dict(a, out=out.data_ptr()), stream=stream)
    vo = v_out.float().cuda().contiguous()
    vpos_w, v_pos = guarded(n * 3)
    vps = [guarded(t.numel(), fill=0.0) for t in tables]
    abi_encode(dict(a, v_out=vo.data_ptr(), v_params=[v[1].data_ptr() for v in vps], v_pos=v_pos.data_ptr()), bwd=True, stream=stream)
    assert guards_intact(out_w, n * W) and guards_intact(vpos_w, n * 3)
    assert all(guards_intact(v[0], t.numel()) for v, t in zip(vps, tables))
    return out.view(n, W).cpu(), [v[1].view_as(t).cpu() for v, t in zip(vps, tables)], v_pos.view(n, 3).cpu()


@functools.lru_cache(maxsize=None)
def reference(F, n, ste):
    """Inputs and float64 results of one case; computed once and shared.  Do not modify."""
    grids = small_grids(F, seed=F, scale=0.7)  # |p| > 1 on ~15 % of the entries: the STE mask matters
    pos = positions(n)
    v_out = torch.randn(n, width(grids), generator=torch.Generator().manual_seed(100 + n), dtype=torch.float64).float()
    v_params, v_pos = HR.encode_backward(pos, grids, v_out, ste)
    return dict(grids=grids, pos=pos, v_out=v_out, out=HR.encode(pos, grids, ste), v_params=v_params, v_pos=v_pos,
                dist=HR.face_distance(pos, grids))


def check_against_reference(label, ref, got):
    out, v_params, v_pos = got
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(v_pos).all())
    assert report(f"{label} forward", rel_l2(out, ref["out"]), BAR) <= BAR
    for i, (g, w) in enumerate(zip(v_params, ref["v_params"])):
        assert report(f"{label} table gradient {i}", rel_l2(g, w), BAR) <= BAR
    keep = ref["dist"] > 1e-5
    assert float((~keep).double().mean()) <= 0.01
    assert report(f"{label} input gradient", rel_l2(v_pos[keep], ref["v_pos"][keep]), BAR) <= BAR


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("F", [1, 2, 4])
def test_encoder_matches_the_float64_restatement(F, n):
    ref = reference(F, n, True)
    got = run_abi(ref["pos"], ref["grids"], True, ref["v_out"])
    check_against_reference(f"F={F} N={n}", ref, got)
    out, _, v_pos = got
    # out-of-range and NaN rows: exactly zero in every grid that reads the bad column, and no gradient into that column
    col = 0
    for g in ref["grids"]:
        w = len(g["resolutions"]) * F
        for r, bad in BAD_AXIS.items():
            if r < n and bad in g["axes"]:
                assert bool((out[r, col:col + w] == 0).all()), (r, g["axes"])
        col += w
    for r, bad in BAD_AXIS.items():
        if r < n:
            assert float(v_pos[r, bad]) == 0.0
            assert bool((out[r] != 0).any())  # (the grid that does not read the bad column still answers)


def test_plain_embeddings_match_the_restatement():
    ref = reference(2, 1000, False)
    check_against_reference("plain F=2 N=1000", ref, run_abi(ref["pos"], ref["grids"], False, ref["v_out"]))


def test_rows_outside_every_grid_contribute_exactly_nothing():
    grids = small_grids(2, seed=3, scale=0.7)
    bad = torch.tensor([-1e-3, 1.001, NAN, -5.0, 1e30])
    pos = bad[torch.randint(0, 5, (300, 3), generator=torch.Generator().manual_seed(2))]
    v_out = torch.randn(300, width(grids), generator=torch.Generator().manual_seed(3))
    out, v_params, v_pos = run_abi(pos, grids, True, v_out)
    assert bool((out == 0).all()) and bool((v_pos == 0).all()) and all(bool((v == 0).all()) for v in v_params)


def test_forward_is_exact_on_dyadic_inputs():
    """(R - 2) powers of two, positions multiples of 2^-6, E = +-1: every product and sum is exact in float32, so where no
    corner is dropped (wn = 1) the forward EQUALS the restatement rounded to float32."""
    F = 2
    grids = small_grids(F, seed=2, scale=1.0)
    assert all(math.log2(r - 2).is_integer() for g in grids for r in g["resolutions"])
    pos = torch.randint(0, 65, (1000, 3), generator=torch.Generator().manual_seed(4)).float() / 64
    out, _, _ = run_abi(pos, grids, True, torch.zeros(1000, width(grids)))
    want = HR.encode(pos, grids, True).float()
    col = checked = 0
    for g in grids:
        for l in range(len(g["resolutions"])):
            one = [dict(g, resolutions=g["resolutions"][l:l + 1], offsets=g["offsets"][l:l + 2])]
            inner = ~HR.has_border_corner(pos, one)
            assert torch.equal(out[inner, col:col + F], want[inner, col:col + F]), (g["axes"], l)
            checked += int(inner.sum())
            col += F
    assert checked > 5000


def test_ste_values_and_gradient_mask():
    from gscodec_studio_amd.compression_simulation import GridEncoder

    enc = GridEncoder(num_dim=2, n_features=1, resolutions_list=(6,), log2_hashmap_size=6).cuda()  # 36 -> 40 rows, dense
    vals = [-1.5, -1.0, -0.0, 0.0, 1.0, 1.5, NAN]
    nodes = [(kx, ky) for ky in range(1, 5) for kx in range(1, 5)][:len(vals)]
    rows = [kx + 6 * ky for kx, ky in nodes]
    with torch.no_grad():
        enc.params.fill_(0.5)
        enc.params[rows, 0] = torch.tensor(vals, device="cuda")
    # u = (k - 0.5) / 4 sits exactly on node k: one corner of weight 1
    pos = torch.tensor([[(kx - 0.5) / 4, (ky - 0.5) / 4] for kx, ky in nodes], device="cuda", requires_grad=True)
    out = enc(pos)
    assert out.shape == (7, 1) and out[:, 0].tolist() == [-1, -1, 1, 1, 1, 1, 0]
    out.sum().backward()
    g = enc.params.grad[:, 0]
    assert g[rows].tolist() == [0, 1, 1, 1, 1, 0, 0]  # zero exactly where |p| > 1 or p is NaN
    assert float(g.sum()) == 4.0 and bool(torch.isfinite(pos.grad).all())


def test_position_gradient_is_deterministic_and_tables_agree():
    ref = reference(2, 1000, True)
    a = run_abi(ref["pos"], ref["grids"], True, ref["v_out"])
    b = run_abi(ref["pos"], ref["grids"], True, ref["v_out"])
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))  # bit-identical: no atomics on this path
    for i, (x, y) in enumerate(zip(a[1], b[1])):  # float atomics reorder the sum
        assert report(f"table gradient {i} run to run", rel_l2(x, y), 1e-5) <= 1e-5


def test_rejections_write_nothing_and_empty_input_launches_nothing():
    from gscodec_studio_amd import _backend as B

    pos = torch.rand(4, 3, device="cuda")
    table = torch.randn(192, 2, device="cuda")
    v_out = torch.randn(4, 4, device="cuda")
    bufs = dict(out=guarded(16), v_pos=guarded(12), v_params=guarded(384))
    base = dict(ENC_BASE, pos=pos.data_ptr(), params=[table.data_ptr()], out=bufs["out"][1].data_ptr(), v_out=v_out.data_ptr(),
                v_params=[bufs["v_params"][1].data_ptr()], v_pos=bufs["v_pos"][1].data_ptr())
    for bwd, extra in ((False, BAD_ENCODE_FWD), (True, BAD_ENCODE_BWD)):
        for over, text in BAD_ENCODE + extra:
            with pytest.raises(RuntimeError, match=rf"status 1.*{text}"):
                abi_encode(dict(base, **over), bwd)
        abi_encode(dict(base, n=0), bwd)
    # the bits kernels: every rule, and empty input
    x, net, hq = torch.randn(4, 3, device="cuda"), torch.rand(4, 6, device="cuda"), torch.full((3,), 0.02, device="cuda")
    bb = dict(bits=guarded(12), v_x=guarded(12), v_net=guarded(24))
    P = {k: v[1].data_ptr() for k, v in bb.items()}
    fa = dict(n=4, C=3, x=x.data_ptr(), net=net.data_ptr(), hq=hq.data_ptr(), bound=1e-6, bits=P["bits"])
    ba = dict(fa, v_bits=x.data_ptr(), v_x=P["v_x"], v_net=P["v_net"])

    def fwd(**o):
        B.call("gs_gaussian_bits_fwd", *[dict(fa, **o)[k] for k in ("n", "C", "x", "net", "hq", "bound", "bits")], None)

    def bwd(**o):
        B.call("gs_gaussian_bits_bwd", *[dict(ba, **o)[k] for k in ("n", "C", "x", "net", "hq", "bound", "v_bits", "v_x", "v_net")], None)

    for fn, ptrs in ((fwd, ("x", "net", "hq", "bits")), (bwd, ("x", "net", "hq", "v_bits", "v_x", "v_net"))):
        for C in (0, 33):
            with pytest.raises(RuntimeError, match=r"status 1.*channels must be in 1\.\.32"):
                fn(C=C)
        for k in ptrs:
            with pytest.raises(RuntimeError, match=r"status 1.*null pointer"):
                fn(**{k: None})
        fn(n=0)
    assert all(untouched(w) for w, _ in list(bufs.values()) + list(bb.values()))
    # and the same arguments, valid, do write (the sentinels above are not there by accident)
    abi_encode(base)
    fwd()
    torch.cuda.synchronize()
    assert not untouched(bufs["out"][0]) and guards_intact(bufs["out"][0], 16)
    assert not untouched(bb["bits"][0]) and guards_intact(bb["bits"][0], 12)


def small_mix(F, seed=0):
    from gscodec_studio_amd.compression_simulation import mix_3D2D_encoding

    mix = mix_3D2D_encoding(F, (4, 6, 10, 18), 7, (6, 10, 34), 6, True, False, False, 1)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, e in mix._encoders():
            e.params.copy_(0.7 * torch.randn(e.params.shape, generator=g))
    return mix.cuda()


@pytest.mark.parametrize("F", [1, 2, 4])
def test_mix_encoding_is_the_four_encoders_concatenated(F):
    mix = small_mix(F)
    pos = positions(1000).cuda().requires_grad_(True)
    out = mix(pos)
    assert out.shape == (1000, 13 * F) == (1000, mix.output_dim)
    pos2 = pos.detach().clone().requires_grad_(True)
    parts = [mix.encoding_xyz(pos2), mix.encoding_xy(pos2[:, [0, 1]]), mix.encoding_xz(pos2[:, [0, 2]]), mix.encoding_yz(pos2[:, [1, 2]])]
    assert torch.equal(out, torch.cat(parts, 1))  # bit for bit
    v_out = torch.randn(out.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out.backward(v_out)
    one = [e.params.grad.clone() for _, e in mix._encoders()]
    mix.zero_grad(set_to_none=True)
    torch.cat(parts, 1).backward(v_out)
    for (name, e), g in zip(mix._encoders(), one):
        assert rel_l2(g, e.params.grad) <= 1e-5, name
    assert rel_l2(pos.grad, pos2.grad) <= 1e-5  # (one sum over 13 levels against four partial sums added by autograd)
    # prefix shapes and a level range
    assert torch.equal(mix(pos.detach().view(10, 100, 3)), out.view(10, 100, -1))
    assert torch.equal(mix.encoding_xyz(pos.detach(), min_level_id=1, max_level_id=3), out[:, F:3 * F])


def test_other_embedding_modes_and_a_side_stream():
    from gscodec_studio_amd.compression_simulation import GridEncoder, STE_multistep

    pos = positions(500).cuda()
    g = torch.Generator().manual_seed(0)
    kw = dict(num_dim=3, n_features=2, resolutions_list=(4, 6, 10, 18), log2_hashmap_size=7)
    plain = GridEncoder(ste_binary=False, **kw)
    with torch.no_grad():
        plain.params.copy_(0.7 * torch.randn(plain.params.shape, generator=g))
    plain = plain.cuda()
    grid = [dict(params=plain.params.detach().cpu(), num_dim=3, axes=(0, 1, 2), resolutions=[4, 6, 10, 18], offsets=plain.offsets_list.tolist())]
    want = plain(pos)
    assert rel_l2(want.cpu(), HR.encode(pos.cpu(), grid, False)) <= BAR
    multi = GridEncoder(ste_binary=False, ste_multistep=True, Q=0.25, **kw).cuda()
    multi.load_state_dict(plain.state_dict())
    q = dict(grid[0], params=STE_multistep.apply(plain.params.detach().cpu(), 0.25))
    assert rel_l2(multi(pos).cpu(), HR.encode(pos.cpu(), [q], False)) <= BAR
    noisy = GridEncoder(ste_binary=False, add_noise=True, Q=4.0, **kw).cuda()
    noisy.load_state_dict(plain.state_dict())
    multi4 = GridEncoder(ste_binary=False, ste_multistep=True, Q=4.0, **kw).cuda()
    multi4.load_state_dict(plain.state_dict())
    assert not torch.equal(noisy(pos), want)  # training: uniform noise of width 1 / Q on the table
    assert torch.equal(noisy(pos, test_phase=True), multi4(pos))  # test phase: the multistep rounding
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = plain(pos)
    side.synchronize()
    assert torch.equal(again, want)
    assert plain(pos[:0]).shape == (0, 8)  # empty input launches nothing


# ---------------------------------------------------------------------------------------------------------------------
# Entropy_gaussian in the reference configuration


@functools.lru_cache(maxsize=None)
def model_case(channel):
    """Module, inputs and the float64 restatement's results; computed once.  Do not modify."""
    from gscodec_studio_amd.compression_simulation import Entropy_gaussian

    torch.manual_seed(channel)
    m = Entropy_gaussian(channel)
    pr = m.param_regressor
    g = torch.Generator().manual_seed(10 + channel)
    encoders = pr.hash_grid._encoders()
    with torch.no_grad():  # parameters scaled up so that the outputs are not ~0; scales around 1
        for _, e in encoders:
            e.params.copy_(0.7 * torch.randn(e.params.shape, generator=g))
        last = pr.mlp_regressor[2]
        last.weight[channel:] *= 0.5
        last.bias[channel:] += 1.0
    n, q = 2000, 12 / 255
    pos = (torch.rand(n, 3, generator=g) * 2 - 1) * 95
    pos[:4] = torch.tensor([[101.0, 0, 0], [0, -100.5, 3], [-100, 100, -100], [100, 100, 100]])
    x = 0.5 * torch.randn(n, channel, generator=g)
    x[::20] += 6.0  # deep in the tail: the likelihood is clamped
    v_bits = torch.rand(n, channel, generator=g) + 0.5
    # float64 restatement: the module's float32 normalisation, then everything in float64
    u = ((pos - pr.bound_min) / (pr.bound_max - pr.bound_min)).requires_grad_(True)
    meta = [dict(num_dim=e.num_dim, axes=AXES_OF[a], resolutions=e.resolutions_list.tolist(), offsets=e.offsets_list.tolist())
            for a, e in encoders]
    tables = [e.params.detach().double().requires_grad_(True) for _, e in encoders]
    mlp = [p.detach().double().requires_grad_(True) for p in pr.mlp_regressor.parameters()]
    sink = {}
    feats = HR.Encode.apply(u, meta, True, sink, *tables)
    net = torch.relu(feats @ mlp[0].T + mlp[1]) @ mlp[2].T + mlp[3]
    xd = x.double().requires_grad_(True)
    bits, like = HR.gaussian_bits_graph(xd, net, q)
    bits.backward(v_bits.double())
    grids = [dict(mt, params=t.detach()) for mt, t in zip(meta, tables)]
    return dict(module=m, pos=pos, x=x, q=q, v_bits=v_bits, bits=bits.detach(), like=like.detach(), net=net.detach(), v_x=xd.grad,
                v_pos=sink["v_pos"] / 200.0, v_tables=[t.grad for t in tables], v_mlp=[p.grad for p in mlp],
                dist=HR.face_distance(u.detach(), grids))


@pytest.mark.parametrize("channel", [3, 4])
def test_entropy_gaussian_reference_configuration(channel):
    ref = model_case(channel)
    m = copy.deepcopy(ref["module"]).cuda()
    x = ref["x"].cuda().requires_grad_(True)
    pos = ref["pos"].cuda().requires_grad_(True)
    bits = m(x, ref["q"], pos=pos)
    assert bits.shape == (2000, channel)
    bits.backward(ref["v_bits"].cuda())
    like, want = ref["like"], ref["bits"]
    assert 0.03 < float((like < 1e-6).double().mean()) < 0.08 and float(ref["net"][:, channel:].min()) > 0.1
    err = (bits.detach().cpu().double() - want).abs()
    bar = 1e-4 * want.abs() + 4e-3
    report(f"Entropy_gaussian({channel}) bits", float((err / bar).max()), 1.0)
    assert bool((err <= bar).all())
    assert report(f"Entropy_gaussian({channel}) v_x", rel_l2(x.grad.cpu(), ref["v_x"]), BAR) <= BAR
    keep = ref["dist"] > 1e-5
    assert float((~keep).double().mean()) <= 0.01
    assert report(f"Entropy_gaussian({channel}) v_pos", rel_l2(pos.grad.cpu()[keep], ref["v_pos"][keep]), BAR) <= BAR
    # outside [-100, 100] in x resp. y: no gradient into that column, the grid that does not read it still answers
    assert float(pos.grad[0, 0]) == 0.0 and float(pos.grad[1, 1]) == 0.0 and bool((pos.grad[0, 1:] != 0).all())
    for (name, e), w in zip(m.param_regressor.hash_grid._encoders(), ref["v_tables"]):
        assert report(f"Entropy_gaussian({channel}) table {name}", rel_l2(e.params.grad.cpu(), w), BAR) <= BAR
    for (name, p), w in zip(m.param_regressor.mlp_regressor.named_parameters(), ref["v_mlp"]):
        assert report(f"Entropy_gaussian({channel}) mlp {name}", rel_l2(p.grad.cpu(), w), BAR) <= BAR
    mean, scale = m.get_means_and_scales(pos.detach())
    assert rel_l2(mean.cpu(), ref["net"][:, :channel]) <= BAR and rel_l2(scale.cpu(), ref["net"][:, channel:]) <= BAR


def test_simulation_estimates_bits_on_the_sample_and_reaches_every_parameter():
    from gscodec_studio_amd.compression_simulation import HashGridCompressionSimulation

    steps = {"means": -1, "scales": 10, "quats": 20, "opacities": -1, "sh0": 30, "shN": -1}
    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda")
    # 4,096 garden points: the fixture holds 4,000, the last 96 are its first 96 again, displaced by 0.01 along every axis
    n, fx = 4096, garden()
    fx = {k: torch.cat([torch.as_tensor(fx[k]), torch.as_tensor(fx[k][:96]) + (0.01 if k == "means" else 0.0)])
          for k in ("means", "scales", "quats", "rgb")}
    g = torch.Generator().manual_seed(0)
    P = lambda t: torch.nn.Parameter(torch.as_tensor(t, dtype=torch.float32).cuda())  # noqa: E731
    splats = {"means": P(fx["means"]), "scales": P(torch.log(torch.as_tensor(fx["scales"]) + 1e-6)), "quats": P(fx["quats"]),
              "opacities": P(torch.randn(n, generator=g)), "sh0": P(torch.as_tensor(fx["rgb"]).view(n, 1, 3)),
              "shN": P(0.05 * torch.randn(n, 15, 3, generator=g))}
    with pytest.raises(RuntimeError, match="_estiblish_bbox"):
        sim.simulate_compression(splats, step=15)
    with torch.no_grad():
        sim._estiblish_bbox(splats["means"])
    out, bits = sim.simulate_compression(splats, step=5)
    assert all(v is None for v in bits.values())
    torch.manual_seed(7)
    out, bits = sim.simulate_compression(splats, step=15)
    torch.manual_seed(7)  # the sample is drawn first, before any quantizer noise
    mask = sim._random_sample_pts(sim._get_pts_inside_bbox(splats["means"]))
    k = int(mask.sum())
    assert 150 <= k <= 215  # 5 % of the ~94 % inside the box
    assert bits["scales"].shape == (k, 3) and all(bits[a] is None for a in ("means", "quats", "opacities", "sh0", "shN"))
    out, bits = sim.simulate_compression(splats, step=35)
    k = bits["scales"].shape[0]
    assert bits["quats"].shape == (k, 4) and bits["sh0"].shape == (k, 3) and bits["opacities"] is None
    assert out["sh0"].shape == (n, 1, 3) and out["scales"].shape == (n, 3) and out["means"].shape == (n, 3)
    assert all(bool(torch.isfinite(b).all()) for b in bits.values() if b is not None)
    sum(b.sum() / b.numel() for b in bits.values() if b is not None).backward()  # the trainer's bpp term
    gm = splats["means"].grad
    assert gm is not None and bool(torch.isfinite(gm).all()) and 0 < int((gm != 0).any(1).sum()) <= k
    for a in ("scales", "quats", "sh0"):
        assert splats[a].grad is not None and float(splats[a].grad.abs().sum()) > 0
        pr = sim.entropy_models[a].param_regressor
        for _, e in pr.hash_grid._encoders():
            assert e.params.grad is not None and float(e.params.grad.abs().sum()) > 0
        for p in pr.mlp_regressor.parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        assert float(pr.mlp_regressor[2].weight.grad.abs().sum()) > 0
        sim.entropy_model_optimizers[a].step()
        sim.entropy_model_schedulers[a].step()
    # activate=True (scales come back exponentiated) keeps working through the base class
    out2, bits2 = sim.simulate_compression(splats, step=35, activate=True)
    assert bool((out2["scales"] > 0).all()) and bits2["quats"].shape[1] == 4 and bits2["scales"].shape[1] == 3


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian bits


def run_bits(x, net, q, v_bits, bound=1e-6):
    from gscodec_studio_amd import _backend as B

    M, C = x.shape
    xt, nt, vb = x.cuda(), net.cuda(), v_bits.cuda()
    hq = torch.full((C,), 0.5 * q, device="cuda")
    (bits_w, bits), (vx_w, v_x), (vn_w, v_net) = guarded(M * C), guarded(M * C), guarded(2 * M * C)
    B.call("gs_gaussian_bits_fwd", M, C, xt.data_ptr(), nt.data_ptr(), hq.data_ptr(), bound, bits.data_ptr(), None)
    B.call("gs_gaussian_bits_bwd", M, C, xt.data_ptr(), nt.data_ptr(), hq.data_ptr(), bound, vb.data_ptr(), v_x.data_ptr(),
           v_net.data_ptr(), None)
    assert guards_intact(bits_w, M * C) and guards_intact(vx_w, M * C) and guards_intact(vn_w, 2 * M * C)
    return bits.view(M, C).cpu(), v_x.view(M, C).cpu(), v_net.view(M, 2 * C).cpu()


def check_bits(label, M, C, seed=0):
    x, net, q = bits_inputs(M, C, seed)
    v_bits = torch.randn(M, C, generator=torch.Generator().manual_seed(seed + 1))
    ref = HR.gaussian_bits(x, net, q, v_bits=v_bits)
    f32 = HR.gaussian_bits(x, net, q, dtype=torch.float32)
    bits, v_x, v_net = run_bits(x, net, q, v_bits)
    like, want = ref["like"], ref["bits"]
    err = (bits.double() - want).abs()
    body = like >= 1e-4
    if body.any():
        bar = 1e-4 * want.abs() + 4e-3
        report(f"{label} bits, likelihood >= 1e-4", float((err / bar)[body].max()), 1.0)
        assert bool((err <= bar)[body].all())
    if (~body).any():  # cancellation territory of the float32 torch form: the kernel may not be worse
        worst, worst32 = float(err[~body].max()), float((f32["bits"].double() - want).abs()[~body].max())
        report(f"{label} bits, likelihood < 1e-4 (float32 torch form: {worst32:.2e})", worst, worst32 + 4e-3)
        assert worst <= worst32 + 4e-3
    near = (like - BOUND).abs() <= 2e-7
    assert float(near.double().mean()) <= 0.01
    clamped = (like < BOUND) & ~near
    if clamped.any():
        assert float((bits[clamped].double() - (-math.log2(1e-6))).abs().max()) <= 1e-4
    for name, got, w, keep in (("v_x", v_x, ref["v_x"], ~near), ("v_net", v_net, ref["v_net"], torch.cat([~near, ~near], 1))):
        assert bool(torch.isfinite(got).all())
        e = float((got.double() - w)[keep].abs().max()) / max(float(w[keep].abs().max()), 1e-30)
        assert report(f"{label} {name}", e, BAR) <= BAR
    return ref, bits, v_x, v_net, v_bits


def test_gaussian_bits_body_tail_clamp_and_gradients():
    ref, bits, v_x, v_net, v_bits = check_bits("bits M=4096 C=4", 4096, 4)
    like = ref["like"]
    assert 0.8 < float((like >= 1e-4).double().mean()) < 0.92 and 0.03 < float((like < 1e-6).double().mean()) < 0.08
    assert bool((v_net[:50, 4:] == 0).all()) and bool((bits[:50] == 0).all())  # raw scale below 1e-9: clamp gate, all the mass in the bin
    blocked = (like < 1e-6 - 2e-7) & (v_bits < 0)  # LowerBound: d loss / d likelihood > 0 at the bound is not passed on
    passing = (like < 1e-6 - 2e-7) & (v_bits > 0)
    assert int(blocked.sum()) > 50 and int(passing.sum()) > 50
    assert bool((v_x[blocked] == 0).all()) and bool((v_x[passing] != 0).any())


@pytest.mark.parametrize("C", [1, 3, 32])
def test_gaussian_bits_shapes(C):
    for M in (1, 63, 65):
        check_bits(f"bits M={M} C={C}", M, C, seed=C + M)
