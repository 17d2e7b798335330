"""Loader of the native C-ABI library ``libgsplat_hip.so`` (ctypes).

Counterpart of the reference's ``gsplat/cuda/_backend.py:79-141`` (which finds or
JIT-builds a pybind11/torch extension).  Here the native side is a plain shared
library with a flat C ABI (``include/gsplat_hip.h``); this module

* loads it from the package tree (``gscodec_studio_amd/csrc/libgsplat_hip.so``),
* reads the header ONCE and derives from that one text everything that crosses the boundary, so the header is the
  single source of truth for the ABI: every function's ctypes prototype (``prototypes()``), the ABI version and the
  header hash, a ``ctypes.Structure`` for every host struct (``struct("gs_step")``: field names, order and types are the
  header's) and every ``#define GS_*`` integer (``const("GS_ROW_FLOATS")``),
* refuses, in ``lib()``, a library whose ABI version, header hash or own ``sizeof`` / ``offsetof`` of the host structs
  (``gs_*_layout``) disagree with that header, before a descriptor is ever handed over,
* exposes ``call(name, *args)`` which passes tensors as raw device pointers, appends
  nothing implicitly, and turns a non-zero status into ``RuntimeError`` with the
  library's ``gs_last_error()`` message.

There is deliberately NO fallback: if the library is missing or a symbol is absent the
import of the op fails loudly (a CPU/eager fallback would silently void every parity
and performance claim made for the HIP path).
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import re
from typing import Dict, List, Optional, Tuple

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_REPO_DIR = os.path.dirname(_PKG_DIR)


def _find_header() -> str:
    """The ABI header: $GSPLAT_HIP_HEADER, the copy the build puts inside the package (``<pkg>/include``, what an
    installed / vendored package carries), or the repository's ``include/`` (source checkout)."""
    cands = [os.environ.get("GSPLAT_HIP_HEADER"), os.path.join(_PKG_DIR, "include", "gsplat_hip.h"),
             os.path.join(_REPO_DIR, "include", "gsplat_hip.h")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    return cands[-1]


HEADER_PATH = _find_header()
LIB_PATH = os.environ.get("GSPLAT_HIP_LIB", os.path.join(_PKG_DIR, "csrc", "libgsplat_hip.so"))

_SCALARS = {
    "uint8_t": ctypes.c_uint8,
    "int32_t": ctypes.c_int32,
    "uint32_t": ctypes.c_uint32,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "size_t": ctypes.c_size_t,
    "float": ctypes.c_float,
    "gs_stream_t": ctypes.c_void_p,
}


def _ctype_of(decl: str):
    """Map one C parameter / return declaration to a ctypes type."""
    decl = decl.strip()
    if "*" in decl:
        if decl.replace("const", "").strip().startswith("char"):
            return ctypes.c_char_p
        return ctypes.c_void_p
    base = decl.replace("const", "").split()[0]
    return _SCALARS[base]


def _parse_prototypes(src: str) -> Dict[str, Tuple[object, List[object], List[str]]]:
    """{function name: (restype, [argtypes], [arg names])} from header text without comments."""
    src = re.sub(r"^\s*#[^\n]*", " ", src, flags=re.M)  # strip preprocessor lines
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(gs_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        ret = ret.replace('extern "C"', "").strip()
        args = " ".join(args.split())
        argtypes, argnames = [], []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                argtypes.append(_ctype_of(a))
                argnames.append(re.findall(r"(\w+)\s*$", a)[0])
        protos[name] = (_ctype_of(ret), argtypes, argnames)
    return protos


def _parse_structs(src: str) -> Dict[str, type]:
    """{struct name: ctypes.Structure subclass} for every ``typedef struct NAME { ... } NAME;`` of header text without
    comments.  Field names, order and types are the header's: scalars of ``_SCALARS``, pointers (any pointee: ``c_void_p``),
    fixed arrays, several declarators per line, ``const``, and an earlier struct by value.  Anything else -- an unknown type, a
    bit-field, a union or nested struct, a function pointer, a preprocessor line inside the body -- is an ImportError naming the
    struct and the declaration: a guessed layout would hand the kernels shifted pointers."""
    structs: Dict[str, type] = {}
    for m in re.finditer(r"\btypedef\s+struct\b\s*(\w*)\s*\{", src):
        name = m.group(1) or "<anonymous>"

        def bad(what: str, decl: str):
            return ImportError(f"gscodec_studio_amd: struct {name} of the ABI header: {what} in `{' '.join(decl.split())}`; "
                               "the ctypes classes are derived from the header and nothing is guessed")

        body, brace, rest = src[m.end():].partition("}")
        tail = re.match(r"\s*(\w+)\s*;", rest)
        if "{" in body or tail is None or tail.group(1) != name:  # (a body without inner braces ends at the first "}")
            raise bad("union, nested struct, unterminated body or a tag that is not the typedef's name", m.group(0) + body + brace + rest[:40])
        fields = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            if re.search(r"^\s*#", decl, flags=re.M):
                raise bad("preprocessor line", decl)
            if ":" in decl:
                raise bad("bit-field", decl)
            if "(" in decl:
                raise bad("function pointer", decl)
            words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split(None, 1)
            if len(words) != 2:
                raise bad("unsupported declarator", decl)
            base, declarators = words
            for d in declarators.split(","):
                f = re.fullmatch(r"\s*((?:\*\s*)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
                if f is None:
                    raise bad("unsupported declarator", decl)
                stars, field, count = f.groups()
                if stars:
                    ct = ctypes.c_void_p
                elif base in _SCALARS or base in structs:
                    ct = _SCALARS.get(base) or structs[base]
                else:
                    raise bad(f"unknown type {base}", decl)
                fields.append((field, ct * int(count) if count else ct))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    return structs


class _Header:
    """One read of the ABI header and everything derived from its text."""

    def __init__(self, path: str):
        try:
            with open(path, "rb") as f:
                raw = f.read()
        except FileNotFoundError as e:
            raise ImportError(
                f"gscodec_studio_amd: ABI header gsplat_hip.h not found (looked at $GSPLAT_HIP_HEADER, "
                f"{os.path.join(_PKG_DIR, 'include')}, {os.path.join(_REPO_DIR, 'include')}); the ctypes prototypes are "
                "derived from it. `make -C gscodec_studio_amd/csrc` copies it into the package.") from e
        # first 8 bytes (big-endian) of the SHA-256 of the file: what the Makefile compiles into gs_header_hash()
        self.hash = int(hashlib.sha256(raw).hexdigest()[:16], 16)
        src = re.sub(r"/\*.*?\*/", " ", raw.decode("utf-8"), flags=re.S)  # strip comments
        src = re.sub(r"//[^\n]*", " ", src)
        self.consts: Dict[str, int] = {k: int(v) for k, v in re.findall(
            r"^[ \t]*#[ \t]*define[ \t]+(GS_\w+)[ \t]+(\d+)[uU]?[ \t]*$", src, flags=re.M)}
        self.structs = _parse_structs(src)
        self.protos = _parse_prototypes(src)


_HEADERS: Dict[str, _Header] = {}


def _header(path: str = HEADER_PATH) -> _Header:
    """The header at ``path``, read and parsed once per process."""
    h = _HEADERS.get(path)
    if h is None:
        h = _HEADERS[path] = _Header(path)
    return h


def parse_header(path: str = HEADER_PATH) -> Dict[str, Tuple[object, List[object], List[str]]]:
    """Return {function name: (restype, [argtypes], [arg names])} for every prototype."""
    return _header(path).protos


def header_abi_version(path: str = HEADER_PATH) -> int:
    """GS_ABI_VERSION as the header declares it."""
    return const("GS_ABI_VERSION", path)


def header_hash(path: str = HEADER_PATH) -> int:
    """First 8 bytes (big-endian) of the SHA-256 of the header file: what the Makefile compiles into gs_header_hash()."""
    return _header(path).hash


def struct(name: str, path: str = HEADER_PATH) -> type:
    """The ``ctypes.Structure`` class of the header's ``typedef struct name`` (built once per header)."""
    try:
        return _header(path).structs[name]
    except KeyError:
        raise ImportError(f"gscodec_studio_amd: {path} does not define struct {name}") from None


def const(name: str, path: str = HEADER_PATH) -> int:
    """The value of the header's ``#define name`` (``GS_*`` integer constants)."""
    try:
        return _header(path).consts[name]
    except KeyError:
        raise ImportError(f"gscodec_studio_amd: {path} does not define {name} (as an integer literal)") from None


# Layout guard: struct -> (the library's gs_*_layout entry, the fields whose offsetof it reports behind sizeof; the lists are the
# ones in the header comments at gs_step_layout and gs_adam_desc_layout)
_LAYOUT_GUARDS = {
    "gs_step": ("gs_step_layout", (
        "C", "sh_K", "eps2d", "tile_size", "sh_mask_logits", "rows_ready", "backgrounds", "radii", "sort_temp_bytes", "block_sums",
        "n_isects", "n_kept_host", "work_bytes", "plan", "scratch", "zero_fill_bytes", "finish_phase", "dyn_motion", "dyn_timestamp",
        "dyn_quant_lo", "dyn_trbf_alive")),
    "gs_quant_desc": ("gs_quant_desc_layout", ("n", "x", "out", "v_out", "v_x", "lo", "q_step", "activation", "philox_offset")),
    "gs_adam_desc": ("gs_adam_desc_layout", (
        "n", "param", "grad", "exp_avg", "exp_avg_sq", "visibility", "rows", "row_width", "lr", "step_size", "mode")),
}


def _check_layout(L: ctypes.CDLL, cls: type, name: str, entry: str, guarded: Tuple[str, ...]) -> None:
    want = (ctypes.c_uint64 * 64)()
    m = int(getattr(L, entry)(want, 64))
    mine = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in guarded]
    if m != len(mine) or list(want[:m]) != mine:
        raise ImportError(f"gscodec_studio_amd: {name}: the class derived from the header does not match the library's "
                          f"struct layout ({entry}: {list(want[:m])} vs {mine}); rebuild with `make -C gscodec_studio_amd/csrc`")


def _check_layouts(L: ctypes.CDLL, structs: Dict[str, type]) -> None:
    for name, (entry, guarded) in _LAYOUT_GUARDS.items():
        _check_layout(L, structs[name], name, entry, guarded)  # (for HEADER_PATH: the very class objects _step, _wrapper and ops hold)


def guarded_struct(name: str, entry: str, guarded: Tuple[str, ...], path: str = HEADER_PATH) -> type:
    """``struct(name)`` after the same check against the library's ``entry`` (sizeof, then the offsetof of ``guarded``): for a
    descriptor whose module guards it itself, before its first table, instead of ``lib()`` at load (``_LAYOUT_GUARDS``)."""
    cls = struct(name, path)
    _check_layout(lib(), cls, name, entry, tuple(guarded))
    return cls


def check_layouts(path: str = HEADER_PATH) -> None:
    """The struct classes derived from the header at ``path`` against the loaded library's own ``sizeof`` / ``offsetof``
    (``gs_step_layout``, ``gs_quant_desc_layout``, ``gs_adam_desc_layout``); ``lib()`` has done this for ``HEADER_PATH``."""
    _check_layouts(lib(), _header(path).structs)


_LIB: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the native library with prototypes attached."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"gscodec_studio_amd: native library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C gscodec_studio_amd/csrc`. There is no CPU fallback."
        )
    hdr = _header()
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes, _) in hdr.protos.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:  # declared in the header but not exported
            raise ImportError(f"gscodec_studio_amd: {LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    # the header the prototypes were parsed from and the library must be the SAME revision of the ABI: the version the
    # header declares, and the hash of the header file the library was compiled against (a changed argument list behind
    # an unchanged version number would otherwise be called through shifted arguments)
    want = header_abi_version()
    if L.gs_version() != want:
        raise ImportError(f"gscodec_studio_amd: ABI version mismatch: {LIB_PATH} reports {L.gs_version()}, "
                          f"{HEADER_PATH} declares {want}; rebuild with `make -C gscodec_studio_amd/csrc`")
    if L.gs_header_hash() != hdr.hash:
        raise ImportError(f"gscodec_studio_amd: {LIB_PATH} was compiled against a different gsplat_hip.h than {HEADER_PATH} "
                          f"(hash {L.gs_header_hash():016x} != {hdr.hash:016x}); rebuild with `make -C gscodec_studio_amd/csrc`")
    # and the host structs that cross the boundary by pointer must be laid out as the library's compiler laid them out
    # (host-only calls; once here, so no call path carries a "checked" flag)
    _check_layouts(L, hdr.structs)
    _LIB = L
    return L


def prototypes() -> Dict:
    lib()
    return _header().protos


def ptr(t) -> Optional[int]:
    """Raw device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def current_stream(device) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def call(name: str, *args) -> None:
    """Call an ``int32_t``-status entry point; raise RuntimeError on failure."""
    L = lib()
    rc = getattr(L, name)(*args)
    if rc != 0:
        msg = L.gs_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (status {rc}): {msg}")


def query(name: str, *args):
    """Call a value-returning helper (e.g. gs_sort_temp_bytes)."""
    return getattr(lib(), name)(*args)
