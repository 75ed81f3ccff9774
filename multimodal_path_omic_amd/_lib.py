"""ctypes binding of libmpo_hip.so (C ABI: include/mpo_hip.h).

Signatures, enum values and the ABI version are read from that header when the module is imported; nothing
here states them a second time.  There is deliberately no fallback: if the shared library is missing or stale,
or a call returns non-zero, a RuntimeError is raised.  Tensors cross the boundary as raw device pointers
(`tensor.data_ptr()`), sizes, and the current HIP stream of the tensor's device.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmpo_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mpo_hip.h")
# Companion headers mpo_hip.h includes (entries added to the ABI after its own list was closed): bound the same way.
COMPANION_HEADER_PATHS = [os.path.join(os.path.dirname(_HERE), "include", name)
                          for name in ("mpo_bag_sample.h", "mpo_fusion_next.h")]
# Headers registered after that list was closed in its turn (companion_symbols() and all_companion_symbols() keep naming what
# they named): same rules, same binding, their own accessor later_symbols().
LATER_HEADER_PATHS = [os.path.join(os.path.dirname(_HERE), "include", name) for name in ("mpo_cohort.h",)]
# Every header registered since (the two lists above are pinned by name in the CPU suite): an open list, one accessor for
# all of it, header_symbols().  A new companion header of mpo_hip.h goes here.
MORE_HEADER_PATHS = [os.path.join(os.path.dirname(_HERE), "include", name) for name in ("mpo_feature_range.h", "mpo_grad_guard.h", "mpo_eval.h",
                                                                                                  "mpo_classify.h", "mpo_patch_f16.h")]

# The closed map from the header's scalar parameter types; a new scalar type in the header needs a new line here.
_SCALARS = {"int": c_int, "int32_t": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float,
            "mpo_stream_t": c_void_p}
_DECL = re.compile(r"^[ \t]*([\w \t*]+?)[ \t]*\b(mpo_\w+)[ \t]*\(([^()]*)\)\s*;", re.M)


def _ctype(entry: str, decl: str):
    """ctypes type of one parameter (or scalar return type) as the header spells it, name optional."""
    if "*" in decl or decl.rstrip().endswith("]"):
        return c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in _SCALARS:
        raise RuntimeError(f"include/mpo_hip.h: {entry}: no ctypes type for '{' '.join(decl.split())}'")
    return _SCALARS[words[0]]


def parse_header(text: str):
    """C header text -> ({entry: (restype, [argtypes])}, {enum constant: value}, MPO_ABI_VERSION or None).  Strict: every
    `mpo_*(` must be one whole declaration `ret name(args);` whose types are all in the map above."""
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+MPO_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
    signatures, parsed = {}, set()
    for m in _DECL.finditer(text):
        ret, name, args = m.groups()
        parsed.add(m.start(2))
        if ret.replace("*", " * ").split() == ["const", "char", "*"]:
            res = c_char_p
        elif "*" in ret:
            raise RuntimeError(f"include/mpo_hip.h: {name}: no ctypes type for the return type '{ret.strip()}'")
        else:
            res = _ctype(name, ret)
        signatures[name] = (res, [] if args.strip() in ("", "void") else [_ctype(name, a) for a in args.split(",")])
    for m in re.finditer(r"\b(mpo_\w+)\s*\(", text):
        if m.start(1) not in parsed:
            raise RuntimeError(f"include/mpo_hip.h: {m.group(1)}: not a whole declaration: "
                               f"'{' '.join(text[m.start():m.start() + 120].split())}'")
    constants = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in body.split(","):
            m = re.fullmatch(r"\s*(MPO_\w+)\s*=\s*(\d+)\s*", item)
            if not m:
                raise RuntimeError(f"include/mpo_hip.h: enum item '{item.strip()}' is not NAME = integer")
            constants[m.group(1)] = int(m.group(2))
    return signatures, constants, int(version.group(1)) if version else None


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the package binds libmpo_hip.so from its public header and ships "
                           "with it (repository layout: include/ beside the package)")
    with open(HEADER_PATH) as f:
        signatures, constants, version = parse_header(f.read())
    if version is None or not signatures:
        raise RuntimeError(f"{HEADER_PATH}: no MPO_ABI_VERSION / no entry declarations found")
    return signatures, constants, version


def _read_companions(paths, taken):
    """Entry signatures of the companion headers `paths` (no enums, no version of their own) -> (all of them, {header: its
    names}).  `taken`: the names declared by the headers read before these; a name declared twice anywhere is an error."""
    out, by_header = {}, {}
    for path in paths:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: include/mpo_hip.h includes it and the package binds its entries")
        with open(path) as f:
            signatures, constants, version = parse_header(f.read())
        if not signatures or constants or version is not None:
            raise RuntimeError(f"{path}: a companion header declares entries only (no enum, no MPO_ABI_VERSION)")
        for name in signatures:
            if name in taken or name in out:
                raise RuntimeError(f"{path}: {name} is declared twice")
        out.update(signatures)
        by_header[os.path.basename(path)] = list(signatures)
    return out, by_header


# Everything below is what include/mpo_hip.h says: the signatures lib() binds, its enums and the ABI version it describes.
_signatures, _constants, ABI_VERSION = _read_header()
MPO_F32, MPO_BF16 = _constants["MPO_F32"], _constants["MPO_BF16"]
ACT = {k[len("MPO_ACT_"):-1].lower(): v for k, v in _constants.items() if k.startswith("MPO_ACT_")}      # MPO_ACT_RELU_ -> relu
OPTIM = {k[len("MPO_OPTIM_"):].lower(): v for k, v in _constants.items() if k.startswith("MPO_OPTIM_")}
GEMM_ROUTE = {k[len("MPO_GEMM_ROUTE_"):].lower(): v for k, v in _constants.items() if k.startswith("MPO_GEMM_ROUTE_")}
_companion_signatures, _companion_names = _read_companions(COMPANION_HEADER_PATHS, _signatures)
_later_signatures, _later_names = _read_companions(LATER_HEADER_PATHS, {**_signatures, **_companion_signatures})
_more_signatures, _more_names = _read_companions(MORE_HEADER_PATHS, {**_signatures, **_companion_signatures, **_later_signatures})


class BagPlanC(ctypes.Structure):
    """mpo_bag_plan of include/mpo_hip.h (host struct; wg_start is a device pointer)."""
    _fields_ = [("wg_start", c_void_p), ("n_wg", ctypes.c_int32), ("rows_per_wg", ctypes.c_int32)]


_REBUILD = "run `python -c 'import __graft_entry__ as g; g.build()'`"
_lib = None


def exported_symbols():
    """Names every build of the library must export (checked by the CPU test-suite): the header's entries."""
    return list(_signatures)


def companion_symbols(header: str = os.path.basename(COMPANION_HEADER_PATHS[0])):
    """The entries declared in the companion header `header` (file name; default: the first, the patch sampler's), in
    the order it declares them: exported and bound like mpo_hip.h's own."""
    return list(_companion_names[header])


def all_companion_symbols():
    """The entries of every companion header (what lib() binds beside exported_symbols())."""
    return list(_companion_signatures)


def later_symbols(header: "str | None" = None):
    """The entries of the headers in LATER_HEADER_PATHS (of one of them, by file name), in declaration order: exported and
    bound like every other entry, named by neither companion_symbols() nor all_companion_symbols()."""
    return list(_later_signatures) if header is None else list(_later_names[header])


def header_symbols(header: str):
    """The entries of the header `header` of MORE_HEADER_PATHS (file name), in declaration order: exported and bound like
    every other entry."""
    return list(_more_names[header])


def check_abi_version(found: int, expected: int):
    if found != expected:
        raise RuntimeError(f"{LIB_PATH} reports ABI version {found}, include/mpo_hip.h describes {expected}: the library is "
                           f"stale ({_REBUILD}). There is no CPU fallback.")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built ({_REBUILD}). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in {**_signatures, **_companion_signatures, **_later_signatures, **_more_signatures}.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        check_abi_version(handle.mpo_abi_version(), ABI_VERSION)
        _lib = handle
    return _lib


def call(name: str, *args):
    """Call the status-returning entry `name`; a non-zero status raises, naming that entry."""
    check(getattr(lib(), name)(*args), name)


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().mpo_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be contiguous and on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libmpo_hip operates on GPU tensors only (got a CPU tensor); there is no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("libmpo_hip needs contiguous tensors")
    return t.data_ptr()


def ptr_array(tensors):
    """ctypes array of device pointers (kept alive by the caller for the duration of the call)."""
    arr = (c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = ptr(t)
    return arr


def stream_of(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def bag_dtype_code(t):
    if t.dtype == torch.float32:
        return MPO_F32
    if t.dtype == torch.bfloat16:
        return MPO_BF16
    raise RuntimeError(f"bag dtype must be float32 or bfloat16, got {t.dtype}")
