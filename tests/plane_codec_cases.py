"""Inputs shared by the plane-codec tests (CPU and GPU): seeded 8-bit planes, the garden splats, and the numpy module's results
for them, computed once per process."""
import functools

import numpy as np

from grid_sort_cases import asset_splats
from gscodec_studio_amd.compression import plane_codec_reference as R

CONTENTS = ("smooth", "noise", "zeros", "full", "checker", "pixel")
# (8, 8): one block; (9, 17): padding in both directions; (24, 24): 9 blocks; (64, 64): exactly S = 4096 symbols per image channel;
# (100, 100): 169 blocks a channel -- with stream_len = 64 a stream is one block, with 4096 one crosses an image-channel boundary
SIZES = ((8, 8), (9, 17), (24, 24), (64, 64), (100, 100))
CHANNELS = (1, 3, 4)
QPS = (0, 4, 22, 37, 51)
STREAM_LENS = (64, 4096)
ODD_STREAM_LEN = 100  # (100, 100) only: streams end inside a block


def plane(content, h, w, ch):
    """uint8 [h, w, ch], seeded by its name and shape."""
    rs = np.random.RandomState(CONTENTS.index(content) * 100003 + h * 1009 + w * 31 + ch)
    if content == "smooth":  # sines plus sigma = 6 noise
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        c = np.arange(ch, dtype=np.float64)[None, None, :]
        v = 128 + 60 * np.sin(y[..., None] / 9.0 + c) + 50 * np.sin(x[..., None] / 13.0 + 2 * c) + 6 * rs.randn(h, w, ch)
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if content == "noise":
        return rs.randint(0, 256, (h, w, ch)).astype(np.uint8)
    if content == "zeros":
        return np.zeros((h, w, ch), np.uint8)
    if content == "full":
        return np.full((h, w, ch), 255, np.uint8)
    if content == "checker":  # the largest AC coefficient there is
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], ch, axis=2)
    p = np.zeros((h, w, ch), np.uint8)  # one bright pixel
    p[h // 2, w // 3] = 255
    return p


def cases():
    """[(name, content, h, w, ch)]: every content at every size, and every channel count at every size and with every content
    (the channel count cycles over the list; a full product would triple the numpy coder's time for no new path)."""
    out = []
    for si, (h, w) in enumerate(SIZES):
        for ci, content in enumerate(CONTENTS):
            ch = CHANNELS[(si + ci) % 3]
            out.append((f"{content}-{h}x{w}x{ch}", content, h, w, ch))
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


def case_plane(case):
    return plane(*case[1:])


@functools.lru_cache(maxsize=None)
def reference_blob(name, qp, stream_len):
    """The numpy module's file for a case (read-only)."""
    blob = R.encode(case_plane(CASES[CASE_IDS.index(name)]), qp, stream_len=stream_len)
    blob.setflags(write=False)
    return blob


@functools.lru_cache(maxsize=None)
def reference_plane(name, qp):
    """The numpy module's reconstruction of a case (read-only)."""
    out = R.reconstruct(case_plane(CASES[CASE_IDS.index(name)]), qp)
    out.setflags(write=False)
    return out


def _morton(means):
    q = np.floor((means - means.min(0)) / (np.ptp(means, axis=0) + 1e-12) * 1023).astype(np.int64)
    key = np.zeros(len(q), np.int64)
    for b in range(10):
        for a in range(3):
            key |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return np.argsort(key, kind="stable")


@functools.lru_cache(maxsize=None)
def garden_splats():
    """The 4,096 garden splats (64 x 64, SH degree 1) every codec test here uses: numpy arrays, read-only."""
    s = asset_splats(4096)
    for v in s.values():
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def garden_planes():
    """{name: uint8 [64, 64, ch]} for scales, quats, opacities, sh0: the garden splats in Morton order of the means, min-max
    quantised to 8 bits per channel in numpy -- the kind of plane ``HevcCompression`` hands the codec (not bit for bit its planes:
    those come from the quantiser kernel, and the GPU tests take them from there)."""
    s = garden_splats()
    order = _morton(s["means"])
    out = {}
    for name in ("scales", "quats", "opacities", "sh0"):
        v = s[name][order].reshape(4096, -1).astype(np.float64)
        if name == "quats":
            v = v / np.linalg.norm(v, axis=1, keepdims=True)
        lo, hi = v.min(0), v.max(0)
        p = np.rint((v - lo) / (hi - lo) * 255).astype(np.uint8).reshape(64, 64, -1)
        p.setflags(write=False)
        out[name] = p
    return out


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))
