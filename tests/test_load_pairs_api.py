"""Host-side checks of cpz_ctx_load_pairs / cpz_ctx_pairs_resident: the header declares both, the
ctypes prototypes follow the header's, the ABI version stays 5, and Gpu.load_pairs /
Gpu.pairs_resident refuse anything but Parameters before the library is called."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpz_ctx_load_pairs", "cpz_ctx_pairs_resident")
# the header's parameter types as the binding declares them (every plain pointer is a void pointer there)
CTYPES = {"cpz_ctx *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "const uint8_t *": ctypes.c_void_p,
          "uint8_t *": ctypes.c_void_p, "size_t *": ctypes.POINTER(ctypes.c_size_t)}


def _header():
    with open(os.path.join(ROOT, "include", "cpz.h")) as f:
        return f.read()


def _params(name):
    """[(type, name)] of the header's declaration of `name`."""
    m = re.search(r"^int %s\(([^)]*)\);" % name, _header(), re.M)
    assert m, "%s is not declared in cpz.h" % name
    out = []
    for part in m.group(1).split(","):
        t = re.match(r"\s*(.*?)(\w+)\s*$", part.replace("\n", " "))
        out.append((t.group(1).strip(), t.group(2)))
    return out


def test_header_declares_both():
    assert _params("cpz_ctx_load_pairs") == [("cpz_ctx *", "ctx"), ("size_t", "npairs"), ("const uint8_t *", "pairs"),
                                             ("size_t *", "built_out")]
    assert _params("cpz_ctx_pairs_resident") == [("cpz_ctx *", "ctx"), ("size_t", "npairs"),
                                                 ("const uint8_t *", "pairs"), ("uint8_t *", "resident_out")]


class _Recorder:
    """Stands in for the library in _native._declare: keeps what is declared per function."""

    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        return self.__dict__["fns"].setdefault(name, types.SimpleNamespace())


def test_prototypes_match_the_header():
    rec = _Recorder()
    _native._declare(rec)
    for name in NAMES:
        assert name in _native.EXPORTED, name
        fn = rec.fns[name]
        assert fn.restype is ctypes.c_int, name
        assert fn.argtypes == [CTYPES[t] for t, _ in _params(name)], (name, fn.argtypes)


def test_abi_version_is_still_5():
    assert _native.ABI_VERSION == 5
    assert re.search(r"^#define\s+CPZ_ABI_VERSION\s+5\b", _header(), re.M)
    m = re.search(r"^#define\s+CPZ_PAIRS_MAX\s+(\d+)", _header(), re.M)
    assert m and int(m.group(1)) == _native.PAIRS_MAX == 64


class _NoLibrary:
    """Any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _gpu_without_library():
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = _NoLibrary()
    g._h = None
    return g


PAIRS = [cp.Parameters(bytes([1 + i]) * 32, bytes([9 + i]) * 32) for i in range(3)]


@pytest.mark.parametrize("bad", [
    PAIRS[0],                                  # one Parameters, not a sequence of them
    [PAIRS[0], (PAIRS[1].g, PAIRS[1].h)],      # a (g, h) tuple
    [PAIRS[0].g + PAIRS[0].h],                 # a 64-byte row
    PAIRS[0].g + PAIRS[0].h,                   # bytes
    [PAIRS[0], None],
    np.zeros((2, 64), np.uint8),               # rows as an array
    7,
    None,
])
@pytest.mark.parametrize("method", ["load_pairs", "pairs_resident"])
def test_wrappers_take_parameters_only(method, bad):
    with pytest.raises(cp.InvalidParams):
        getattr(_gpu_without_library(), method)(bad)


def test_wrappers_pass_rows_and_counts_on():
    seen = {}

    class Lib:
        def cpz_ctx_load_pairs(self, h, npairs, gh, built):
            seen["load"] = (npairs, bytes((ctypes.c_uint8 * (64 * npairs)).from_address(gh)))
            built._obj.value = 2
            return 0

        def cpz_ctx_pairs_resident(self, h, npairs, gh, out):
            seen["resident"] = (npairs, bytes((ctypes.c_uint8 * (64 * npairs)).from_address(gh)))
            (ctypes.c_uint8 * npairs).from_address(out)[1] = 1
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    rows = b"".join(p.g + p.h for p in PAIRS)
    assert g.load_pairs(PAIRS) == 2
    res = g.pairs_resident(PAIRS)
    assert res.dtype == np.bool_ and res.tolist() == [False, True, False]
    assert seen == {"load": (3, rows), "resident": (3, rows)}
