"""Host-side checks of cpz_verify_batch_pairs_many / Gpu.verify_batch_pairs_many: the header
declares the entry point and its bound and says what the call does above CPZ_PAIRS_MAX pairs, the
ctypes prototype follows the header's, the ABI version stays 5, the built library exports the
symbol, and the wrapper checks its indices before the library is called."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cpz_verify_batch_pairs_many"
CTYPES = {"cpz_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
          "const uint8_t *": ctypes.c_void_p, "const uint32_t *": ctypes.c_void_p, "const uint64_t *": ctypes.c_void_p,
          "uint64_t": ctypes.c_uint64, "uint8_t *": ctypes.c_void_p, "int *": ctypes.POINTER(ctypes.c_int),
          "const uint8_t [32]": ctypes.c_void_p, "uint8_t [32]": ctypes.c_void_p}


def _header():
    with open(os.path.join(ROOT, "include", "cpz.h")) as f:
        return f.read()


def _params(name):
    """[(type, name)] of the header's declaration of `name`; an array parameter's type carries its bound."""
    m = re.search(r"^int %s\(([^)]*)\);" % name, _header(), re.M)
    assert m, "%s is not declared in cpz.h" % name
    out = []
    for part in m.group(1).split(","):
        part = part.replace("\n", " ").strip()
        arr = re.match(r"(.*?)(\w+)(\[\d+\])$", part)
        if arr:
            out.append((arr.group(1).strip() + " " + arr.group(3), arr.group(2)))
        else:
            t = re.match(r"(.*?)(\w+)$", part)
            out.append((t.group(1).strip(), t.group(2)))
    return out


def test_header_declares_the_entry_point_like_its_sibling():
    many, ex = _params(NAME), _params("cpz_verify_batch_pairs_ex")
    assert many == ex
    assert [n for _, n in many] == ["ctx", "flags", "npairs", "pairs", "n", "pair_idx", "y1", "y2", "r1", "r2", "s",
                                    "ctx_bytes", "ctx_off", "ctx_present", "seed", "first_index", "partial_out",
                                    "batch_ok", "status_out"]


def test_header_constant_and_comment():
    src = _header()
    m = re.search(r"^#define\s+CPZ_BATCH_PAIRS_MANY_MAX\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) == _native.BATCH_PAIRS_MANY_MAX == 4096
    # the comment that precedes the declaration
    end = src.index("#define CPZ_BATCH_PAIRS_MANY_MAX")
    comment = src[src.rindex("/*", 0, end):end]
    flat = " ".join(comment.replace("*", " ").split())
    for phrase in ("CPZ_BATCH_PAIRS_MANY_MAX", "npairs <= CPZ_PAIRS_MAX is cpz_verify_batch_pairs_ex itself",
                   "CPZ_CALL_PARTITIONED is ignored", "builds no table", "cpz_combine_partials", "Host buffers only",
                   "CPZ_FALLBACK_NONE or _BISECTION", "no output buffer is written"):
        assert phrase in flat, phrase
    # the sibling keeps its own bound
    assert "npairs > CPZ_PAIRS_MAX" in src


def test_prototype_matches_the_header():
    class Recorder:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            return self.__dict__["fns"].setdefault(name, types.SimpleNamespace())

    rec = Recorder()
    _native._declare(rec)
    assert NAME in _native.EXPORTED
    fn = rec.fns[NAME]
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [CTYPES[t] for t, _ in _params(NAME)], fn.argtypes
    assert fn.argtypes == rec.fns["cpz_verify_batch_pairs_ex"].argtypes


def test_abi_version_is_still_5():
    assert _native.ABI_VERSION == 5
    assert re.search(r"^#define\s+CPZ_ABI_VERSION\s+5\b", _header(), re.M)


def test_built_library_exports_the_entry_point():
    assert os.path.exists(_native.LIB_PATH), "build() leaves the library in the tree"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, NAME)
    assert lib.cpz_abi_version() == 5


class _NoLibrary:
    """Any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _gpu_without_library():
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = _NoLibrary()
    g._h = None
    return g


NP = 70
N = 6
ROWS = [np.zeros((N, 32), np.uint8) for _ in range(5)]
PAIRS = [cp.Parameters(bytes([1 + i]) * 32, bytes([101 + i]) * 32) for i in range(NP)]
SEED = bytes(range(32))


@pytest.mark.parametrize("idx", [
    [0, 1, 2, 3, 69],                          # too short
    [0, 1, 2, 3, 4, 5, 6],                     # too long
    [[0, 1, 2], [3, 4, 5]],                    # not one-dimensional
    [0, 1, 70, 0, 1, 2],                       # 70 is not below the 70 pairs
    [0, -1, 2, 0, 1, 2],                       # negative
    np.array([0, 1, 2 ** 32, 0, 1, 2], np.int64),   # would wrap to 0 as uint32
    [0.0, 1.0, 2.0, 0.0, 1.0, 2.0],            # not integers
    [True, False, True, False, True, False],   # not integers
])
def test_bad_pair_idx_is_rejected_before_the_library_is_called(idx):
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_batch_pairs_many(PAIRS, idx, *ROWS, SEED)


def test_row_shapes_are_checked_before_the_library_is_called():
    rows = [r.copy() for r in ROWS]
    rows[3] = np.zeros((N - 1, 32), np.uint8)
    with pytest.raises(ValueError):   # as every wrapper's row check reports it
        _gpu_without_library().verify_batch_pairs_many(PAIRS, [0] * N, *rows, SEED)


@pytest.mark.parametrize("statuses", [True, False])
def test_good_arguments_reach_the_library(statuses):
    seen = {}

    class Lib:
        def cpz_verify_batch_pairs_many(self, h, flags, npairs, gh, n, idx, y1, y2, r1, r2, s, cb, co, cpres, seed,
                                        first_index, partial, ok, status):
            seen.update(flags=flags, npairs=npairs, n=n, seed=seed, first_index=first_index, status=status is not None,
                        gh=ctypes.string_at(gh, 64 * npairs),
                        idx=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(idx)).tolist())
            ctypes.memmove(partial, bytes([7]) * 32, 32)
            ok._obj.value = 1
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    partial, ok, st = g.verify_batch_pairs_many(PAIRS, np.array([69, 0, 1, 2, 69, 5], np.int64), *ROWS, SEED,
                                                first_index=77, statuses=statuses, equations_only=True)
    assert seen == {"flags": _native.CALL_EQUATIONS_ONLY, "npairs": NP, "n": N, "idx": [69, 0, 1, 2, 69, 5],
                    "seed": SEED, "first_index": 77, "status": statuses, "gh": b"".join(p.g + p.h for p in PAIRS)}
    assert partial == bytes([7]) * 32 and ok is True
    assert (st is not None) == statuses and (st is None or st.shape == (N,))
