"""Hand-built .ply files shared by the PLY tests (CPU and GPU): property layouts, seeded payloads, and the oracle -- numpy's own
reading of the rows followed by the column statements of the reference's ``load_ply`` (examples/simple_trainer.py:460-508)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ply.npz")

# PLY scalar type (either spelling) -> numpy format; written out here, not taken from the package under test
NUMPY_OF = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
            "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8",
            "float64": "<f8"}
LAYOUTS = ("standard", "no_normals", "shuffled", "double", "uchar_front", "extra40")
SHN_COEFFS = (0, 3, 15, 24)
SIZES = (1, 255, 256, 257, 1000)
KEYS = ("means", "sh0", "shN", "opacities", "scales", "quats")


def standard_names(kn, normals=True, k0=1, S=3, Q=4):
    return (["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + [f"f_dc_{i}" for i in range(3 * k0)]
            + [f"f_rest_{i}" for i in range(3 * kn)] + ["opacity"] + [f"scale_{i}" for i in range(S)] + [f"rot_{i}" for i in range(Q)])


def layout(kind, kn):
    """[(type, name)] of the vertex element."""
    props = [("float", n) for n in standard_names(kn, normals=kind != "no_normals")]
    if kind == "shuffled":
        order = np.random.RandomState(100 + kn).permutation(len(props))
        props = [props[i] for i in order]
    elif kind == "double":
        props = [("float64" if n == "opacity" else "double" if n.startswith("scale_") else t, n) for t, n in props]
    elif kind == "uchar_front":
        props = [("uchar", "red"), ("uint8", "green"), ("uchar", "blue")] + props
    elif kind == "extra40":
        extra = [("float32", f"extra_{i}") for i in range(40)]
        props = props[:3] + extra[:20] + props[3:] + extra[20:]
    return props


def header_bytes(n, props, newline="\n", comments=(), after=""):
    lines = ["ply", "format binary_little_endian 1.0"] + list(comments) + [f"element vertex {n}"]
    lines += [f"property {t} {name}" for t, name in props]
    if after:
        lines += after.split("\n")
    return (newline.join(lines + ["end_header"]) + newline).encode("ascii")


def dtype_of(props):
    """The packed structured dtype of a row, from the property list alone."""
    return np.dtype([(name, NUMPY_OF[t]) for t, name in props])


def payload(n, props, seed=0):
    rs = np.random.RandomState(seed)
    rows = np.zeros(n, dtype_of(props))
    for t, name in props:
        fmt = np.dtype(NUMPY_OF[t])
        rows[name] = rs.randint(0, 200, n).astype(fmt) if fmt.kind in "iu" else rs.standard_normal(n).astype(fmt)
    return rows


def reference_columns(v):
    """The statements of the reference's ``load_ply`` on a structured array ``v``: float64 column copies, the channel-major
    reshape, float32 at the end."""
    names = v.dtype.names
    n = len(v)
    means = np.stack((v["x"], v["y"], v["z"]), axis=1)

    def group(prefix):
        size = len([p for p in names if p.startswith(prefix)])
        data = np.zeros((n, size))
        for i in range(size):
            data[:, i] = v[f"{prefix}{i}"]
        return data

    sh0, shN = group("f_dc_"), group("f_rest_")
    # (the reference writes reshape(-1, ...), which numpy cannot resolve for a group of no columns; n says the same)
    sh0 = sh0.reshape(n, 3, sh0.shape[1] // 3).transpose(0, 2, 1)
    shN = shN.reshape(n, 3, shN.shape[1] // 3).transpose(0, 2, 1)
    opacities = v["opacity"].reshape(-1, 1)
    return {"means": means.astype(np.float32), "sh0": sh0.astype(np.float32), "shN": shN.astype(np.float32),
            "opacities": opacities.astype(np.float32).squeeze(1), "scales": group("scale_").astype(np.float32),
            "quats": group("rot_").astype(np.float32)}


def oracle(file_bytes, header):
    """The six arrays of a file: ``np.frombuffer`` with the dtype built from the parsed header's names / types / offsets, then
    ``reference_columns``."""
    dt = np.dtype({"names": [p.name for p in header.properties], "formats": [NUMPY_OF[p.type] for p in header.properties],
                   "offsets": [p.offset for p in header.properties], "itemsize": header.stride})
    return reference_columns(np.frombuffer(file_bytes, dt, count=header.count, offset=header.payload_offset))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
