"""float64 torch restatement of the hash-grid Gaussian entropy model (csrc/hashgrid.hip), written from the description of
its semantics: encoder forward, table gradient with the STE mask, the reference-formula input gradient, and the Gaussian
bits through torch.distributions.Normal with the LowerBound and clamp rules.  Test infrastructure (CPU tensors only).

A grid is a dict: params [rows, F], num_dim (2 | 3), axes (columns of the positions), resolutions, offsets.

Per (point, level), R the resolution, T = offsets[l+1] - offsets[l]:
  * a coordinate outside [0, 1] or NaN: zero outputs, no gradient;
  * p = u * float(R - 2) + 0.5f -- for float32 positions in float32 with two roundings (what decides the cell a point falls
    into is part of the semantics), for float64 positions in float64 (differentiable); g = floor(p), f = p - g in float64;
  * corner i: c[d] = g[d] or min(g[d] + 1, R - 1) by bit d of i, w = prod(bit ? f : 1 - f); a corner with a c[d] in {0, R - 1}
    takes no part; row = (dense index while the stride fits T, else xor c[d] * prime[d], uint32 arithmetic) % T;
  * out = sum w / wn * E[row], wn = sum of the participating w (1e-9 if 0); E = (p >= 0) - (p < 0) under STE_binary, else p;
  * table gradient: w / wn * v_out, times (-1 <= p <= 1) under STE_binary;
  * input gradient (NOT the derivative of the renormalised forward near the border): for axis gd the sum over channels and
    the 2^(D-1) corner pairs of v_out * float(R - 2) * prod_{d != gd}(weight) * (E_right - E_left), a border corner counting as 0.
"""
import torch

PRIMES = (1, 2654435761, 805459861)
M32 = 0xFFFFFFFF
SCALE_MIN = 1e-9


def embed(params, ste_binary):
    p = params.double()
    return (p >= 0).double() - (p < 0).double() if ste_binary else p


def ste_mask(params, ste_binary):
    return ((params >= -1) & (params <= 1)).double() if ste_binary else torch.ones_like(params, dtype=torch.float64)


def _rows(c, R, T):
    """c: list of D int64 tensors -> row inside the level's slice."""
    stride, index = 1, torch.zeros_like(c[0])
    for cd in c:
        if stride <= T:
            index = (index + cd * stride) & M32
            stride = (stride * R) & M32
    if stride > T:
        index = torch.zeros_like(c[0])
        for cd, prime in zip(c, PRIMES):
            index = index ^ ((cd * prime) & M32)
    return index % T


def levels(pos, grid):
    """Per level of one grid: dict(R, D, oob [N], f [N, D], w / live / rows [N, 2^D] (rows: global into params))."""
    D, axes = grid["num_dim"], list(grid["axes"])
    u = pos[:, axes]
    oob = ~((u >= 0) & (u <= 1)).all(1)
    u = torch.where(oob[:, None], torch.full_like(u, 0.5), u)
    for l, R in enumerate(grid["resolutions"]):
        off, T = grid["offsets"][l], grid["offsets"][l + 1] - grid["offsets"][l]
        if u.dtype == torch.float32:
            p = (u * torch.tensor(float(R - 2), dtype=torch.float32) + torch.tensor(0.5, dtype=torch.float32)).double()
        else:
            p = u * float(R - 2) + 0.5
        g = torch.floor(p.detach())
        f, gi = p - g, g.long()
        w, live, rows = [], [], []
        for i in range(1 << D):
            c, wi, border = [], torch.ones_like(f[:, 0]), torch.zeros_like(oob)
            for d in range(D):
                bit = (i >> d) & 1
                cd = torch.clamp(gi[:, d] + 1, max=R - 1) if bit else gi[:, d]
                wi = wi * (f[:, d] if bit else 1 - f[:, d])
                border = border | (cd == 0) | (cd == R - 1)
                c.append(cd)
            w.append(wi)
            live.append(~border)
            rows.append(off + _rows(c, R, T))
        yield dict(R=R, D=D, axes=axes, oob=oob, f=f, w=torch.stack(w, 1), live=torch.stack(live, 1), rows=torch.stack(rows, 1))


def encode(pos, grids, ste_binary=True):
    """-> out [N, levels * F] float64; differentiable in ``pos`` when it is float64 (the derivative of the forward itself)."""
    outs = []
    for grid in grids:
        E = embed(grid["params"], ste_binary)
        for lv in levels(pos, grid):
            wl = lv["w"] * lv["live"]
            wn = wl.sum(1, keepdim=True)
            wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
            out = ((wl / wn)[:, :, None] * E[lv["rows"]]).sum(1)
            outs.append(torch.where(lv["oob"][:, None], torch.zeros_like(out), out))
    return torch.cat(outs, 1)


def encode_backward(pos, grids, v_out, ste_binary=True):
    """-> ([v_params per grid], v_pos [N, pos_dim]) float64: table gradient and the reference-formula input gradient."""
    v_out = v_out.double()
    v_pos = torch.zeros(pos.shape, dtype=torch.float64)
    v_params, col = [], 0
    for grid in grids:
        F = grid["params"].shape[1]
        E, mask = embed(grid["params"], ste_binary), ste_mask(grid["params"], ste_binary)
        vt = torch.zeros(grid["params"].shape, dtype=torch.float64)
        for lv in levels(pos, grid):
            D, R, f = lv["D"], lv["R"], lv["f"].detach()
            vo = v_out[:, col:col + F] * (~lv["oob"])[:, None]
            col += F
            wl = lv["w"].detach() * lv["live"]
            wn = wl.sum(1, keepdim=True)
            wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
            coef = wl / wn
            for i in range(1 << D):
                vt.index_add_(0, lv["rows"][:, i], coef[:, i, None] * vo * mask[lv["rows"][:, i]])
            Ec = E[lv["rows"]] * lv["live"][:, :, None]  # [N, 2^D, F], a border corner counts as 0
            for gd in range(D):
                acc = torch.zeros_like(f[:, 0])
                for i in range(1 << D):
                    if (i >> gd) & 1:
                        continue
                    wp = torch.full_like(acc, float(R - 2))
                    for d in range(D):
                        if d != gd:
                            wp = wp * (f[:, d] if (i >> d) & 1 else 1 - f[:, d])
                    acc = acc + wp * (vo * (Ec[:, i | (1 << gd)] - Ec[:, i])).sum(1)
                v_pos[:, lv["axes"][gd]] += acc
        v_params.append(vt)
    return v_params, v_pos


def face_distance(pos, grids):
    """[N]: smallest distance (in cells) of a point to a cell face over all levels; inf for a point no level evaluates."""
    dist = torch.full((pos.shape[0],), float("inf"), dtype=torch.float64)
    for grid in grids:
        for lv in levels(pos, grid):
            f = lv["f"].detach()
            d = torch.minimum(f, 1 - f).min(1).values
            dist = torch.minimum(dist, torch.where(lv["oob"], torch.full_like(d, float("inf")), d))
    return dist


def has_border_corner(pos, grids):
    """[N] bool: some level drops a corner of the point's cell (renormalisation at work)."""
    hit = torch.zeros(pos.shape[0], dtype=torch.bool)
    for grid in grids:
        for lv in levels(pos, grid):
            hit |= ~lv["live"].all(1) & ~lv["oob"]
    return hit


class Encode(torch.autograd.Function):
    """The encoder as the kernels define it: forward ``encode``, backward ``encode_backward`` (float32 positions)."""

    @staticmethod
    def forward(ctx, pos, meta, ste_binary, sink, *params):
        ctx.pos, ctx.meta, ctx.ste, ctx.sink, ctx.params = pos.detach(), meta, ste_binary, sink, [p.detach() for p in params]
        return encode(ctx.pos, [dict(m, params=p) for m, p in zip(meta, ctx.params)], ste_binary)

    @staticmethod
    def backward(ctx, v_out):
        v_params, v_pos = encode_backward(ctx.pos, [dict(m, params=p) for m, p in zip(ctx.meta, ctx.params)], v_out, ctx.ste)
        ctx.sink["v_pos"] = v_pos  # float64 (autograd hands the positions' own dtype on)
        return (v_pos.to(ctx.pos.dtype), None, None, None) + tuple(v_params)


class _LowerBound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ((x >= ctx.bound) | (g < 0)) * g, None


def gaussian_bits_graph(x, net, q, bound=1e-6):
    """-> (bits, likelihood before the bound), differentiable: the module's torch form (Normal.cdf differences)."""
    C = x.shape[1]
    scale = torch.clamp(net[:, C:], min=SCALE_MIN)
    m1 = torch.distributions.normal.Normal(net[:, :C], scale)
    like = torch.abs(m1.cdf(x + 0.5 * q) - m1.cdf(x - 0.5 * q))
    return -torch.log2(_LowerBound.apply(like, bound)), like


def gaussian_bits(x, net, q, bound=1e-6, v_bits=None, dtype=torch.float64):
    """-> dict(bits, like, v_x, v_net) in ``dtype``."""
    x = x.detach().to(dtype).requires_grad_(True)
    net = net.detach().to(dtype).requires_grad_(True)
    bits, like = gaussian_bits_graph(x, net, q, bound)
    res = dict(bits=bits.detach(), like=like.detach())
    if v_bits is not None:
        bits.backward(v_bits.to(dtype))
        res.update(v_x=x.grad, v_net=net.grad)
    return res
