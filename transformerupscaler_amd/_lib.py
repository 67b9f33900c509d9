"""ctypes binding of libtupscale_hip.so, derived at import from include/tupscale_hip.h (the one statement of the C ABI).

There is deliberately no fallback: if the library is missing or a symbol is absent the
import fails loudly, and every call checks the returned hipError_t.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_double, c_float, c_int, c_longlong, c_uint, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TUP_LIB_PATH") or os.path.join(_HERE, "libtupscale_hip.so")      # override: A/B of two builds

P = c_void_p
I = c_int
F = c_float
U = c_uint


class TupscaleLibraryError(RuntimeError):
    pass


_SCALARS = {"int": I, "long long": c_longlong, "float": F, "double": c_double, "unsigned int": U}


def _parse_header(text):
    """The C ABI as the header declares it: ({name: argtypes}, {name: restype}, TUP_ABI_VERSION).  Anything between the
    comments that is not `(int|long long) tup_x(args);` with pointer or known scalar parameters is an error, never a guess."""
    version = re.search(r"^#define\s+TUP_ABI_VERSION\s+(\d+)\s*$", text, re.M)
    if not version:
        raise TupscaleLibraryError("the header does not define TUP_ABI_VERSION")
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", " ", text, flags=re.S | re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    signatures, restypes = {}, {}
    for proto in filter(None, (" ".join(p.split()) for p in text.split(";"))):
        m = re.fullmatch(r"(int|long long) (tup_\w+) ?\((.*)\)", proto)
        if not m:
            raise TupscaleLibraryError(f"cannot split the prototype {proto!r}")
        argtypes = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            kind = re.sub(r"\bconst\b", " ", param).split()[:-1]          # the type's words; the last word is the name
            if "*" in param:
                argtypes.append(P)
            elif " ".join(kind) in _SCALARS:
                argtypes.append(_SCALARS[" ".join(kind)])
            else:
                raise TupscaleLibraryError(f"unknown scalar type in parameter {param.strip()!r} of {m.group(2)}")
        signatures[m.group(2)], restypes[m.group(2)] = argtypes, _SCALARS[m.group(1)]
    if not signatures:
        raise TupscaleLibraryError("the header declares no tup_* entry")
    return signatures, restypes, int(version.group(1))


# name -> argtypes, name -> restype (c_longlong: an element count, not a hipError_t) and the ABI number, all from the one header
with open(os.path.join(_HERE, "..", "include", "tupscale_hip.h")) as _f:
    SIGNATURES, RESTYPES, ABI_VERSION = _parse_header(_f.read())

_lib = None


def load():
    """Load the HIP library once; raise TupscaleLibraryError (never fall back) if unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TupscaleLibraryError(
            f"{LIB_PATH} not found: build it with `make -C transformerupscaler_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    # The kernels must run in the same HIP runtime instance as the device memory and streams they are
    # handed.  torch bundles its own libamdhip64; importing it first makes the dynamic loader resolve our
    # DT_NEEDED libamdhip64.so.N to that already-loaded copy instead of a second runtime from /opt/rocm.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise TupscaleLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    if lib.tup_abi_version() != ABI_VERSION:
        raise TupscaleLibraryError(f"ABI mismatch: library {lib.tup_abi_version()} != binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


_fns = {}


def call(name: str, *args):
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    err = fn(*args)
    if err != 0:
        raise RuntimeError(f"{name} failed with hipError_t {err}")
