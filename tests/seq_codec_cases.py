"""Inputs shared by the plane-sequence codec tests (CPU and GPU): seeded 8-bit sequences built on ``plane_codec_cases.plane``, the
drifting garden planes of the rate condition, and the numpy module's results for them, computed once per process."""
import functools

import numpy as np

from plane_codec_cases import garden_planes, plane
from gscodec_studio_amd.compression import plane_seq_codec_reference as R

# "drift": a smooth plane plus accumulated N(0, 1.5) noise per frame; "noise": independent frames; "flip": zeros and 255 alternating
# (residuals of +-255, the largest DC); "checker-flip": the checker and its inverse alternating (the largest AC residual, both clips)
CONTENTS = ("drift", "noise", "flip", "checker-flip")
# (8, 8): one block; (9, 17): padding in both directions; (24, 24): 9 blocks; (100, 100): 169 blocks a channel, so three channels
# span two workgroups, the second partial
SIZES = ((8, 8), (9, 17), (24, 24), (100, 100))
FRAMES = (1, 2, 5)
CHANNELS = (1, 3, 4)
QPS = (0, 22, 51)
STREAM_LENS = (64, 4096)
DRIFT_SIGMA = 1.5
RATE_SEED, RATE_FRAMES = 20240611, 6


def drift(base, frames, rs, sigma=DRIFT_SIGMA):
    """uint8 [frames, ...]: ``base`` plus a random walk of N(0, sigma) grey levels per frame, rounded and clipped."""
    walk = np.cumsum(rs.randn(frames, *base.shape) * sigma, axis=0)
    walk[0] = 0
    return np.clip(np.rint(base.astype(np.float64)[None] + walk), 0, 255).astype(np.uint8)


def sequence(content, h, w, ch, frames):
    """uint8 [frames, h, w, ch], seeded by its name and shape."""
    rs = np.random.RandomState(CONTENTS.index(content) * 7919 + h * 1009 + w * 31 + ch * 7 + frames)
    if content == "drift":
        return drift(plane("smooth", h, w, ch), frames, rs)
    if content == "noise":
        return rs.randint(0, 256, (frames, h, w, ch)).astype(np.uint8)
    pair = (plane("zeros", h, w, ch), plane("full", h, w, ch)) if content == "flip" else (plane("checker", h, w, ch), 255 - plane("checker", h, w, ch))
    return np.stack([pair[t % 2] for t in range(frames)])


def cases():
    """[(name, content, h, w, ch, frames, gop)]: every content at every size with every frame count; the channel count and the gop
    (1, 2, 3, T + 1) cycle so that each meets every frame count (a full product would take the numpy coder minutes for no new path)."""
    out, i = [], 0
    for content in CONTENTS:
        for h, w in SIZES:
            for frames in FRAMES:
                ch, gop = CHANNELS[(i + i // 3) % 3], (1, 2, 3, frames + 1)[i % 4]
                out.append((f"{content}-{frames}x{h}x{w}x{ch}-gop{gop}", content, h, w, ch, frames, gop))
                i += 1
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


def case_of(name):
    return CASES[CASE_IDS.index(name)]


@functools.lru_cache(maxsize=None)
def case_frames(name):
    out = sequence(*case_of(name)[1:6])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_levels(name, qp):
    """The numpy module's (levels, decoded frames) of a case (read-only)."""
    out = R._closed_loop(R.check_frames(case_frames(name), qp, case_of(name)[6]), qp, case_of(name)[6])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_blob(name, qp, stream_len):
    """The numpy module's file for a case (read-only)."""
    blob = R.encode(case_frames(name), qp, case_of(name)[6], stream_len=stream_len)
    blob.setflags(write=False)
    return blob


@functools.lru_cache(maxsize=None)
def garden_sequences():
    """{name: uint8 [6, 64, 64, ch]}: the four ``garden_planes()`` attributes drifting by sigma = 1.5 a frame -- the input of the
    rate condition."""
    rs = np.random.RandomState(RATE_SEED)
    out = {}
    for name, p in garden_planes().items():
        out[name] = drift(p, RATE_FRAMES, rs)
        out[name].setflags(write=False)
    return out
