"""Host-side checks of cpz_verify_each_gh / cpz_verify_each_gh_device / cpz_challenges_gh and their
wrappers: the header declares the three entry points and CPZ_STATUS_BAD_GENERATOR and says what the
calls do, the ctypes prototypes follow the header's, the ABI version stays 5, the built library
exports the symbols, the Rust declarations are there, and the wrappers check shapes and lengths
before the library is called."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE, CHAL = "cpz_verify_each_gh", "cpz_verify_each_gh_device", "cpz_challenges_gh"
CTYPES = {"cpz_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
          "const uint8_t *": ctypes.c_void_p, "const uint64_t *": ctypes.c_void_p, "uint8_t *": ctypes.c_void_p,
          "const void *": ctypes.c_void_p, "void *": ctypes.c_void_p}


def _header():
    with open(os.path.join(ROOT, "include", "cpz.h")) as f:
        return f.read()


def _params(name):
    """[(type, name)] of the header's declaration of `name`."""
    m = re.search(r"^int %s\(([^)]*)\);" % name, _header(), re.M)
    assert m, "%s is not declared in cpz.h" % name
    out = []
    for part in m.group(1).split(","):
        t = re.match(r"(.*?)(\w+)$", part.replace("\n", " ").strip())
        out.append((t.group(1).strip(), t.group(2)))
    return out


def test_header_declares_the_three_entry_points():
    assert _params(HOST) == [("cpz_ctx *", "ctx"), ("uint32_t", "flags"), ("size_t", "n")] + [
        ("const uint8_t *", q) for q in ("g", "h", "y1", "y2", "r1", "r2", "s", "ctx_bytes")] + [
        ("const uint64_t *", "ctx_off"), ("const uint8_t *", "ctx_present"), ("uint8_t *", "status_out")]
    assert _params(DEVICE) == [("cpz_ctx *", "ctx"), ("uint32_t", "flags"), ("size_t", "n")] + [
        ("const void *", q) for q in ("d_g", "d_h", "d_y1", "d_y2", "d_r1", "d_r2", "d_s", "d_ctx_bytes")] + [
        ("const uint64_t *", "d_ctx_off"), ("const uint8_t *", "d_ctx_present"), ("void *", "d_status_out"),
        ("void *", "stream")]
    assert _params(CHAL) == [("cpz_ctx *", "ctx"), ("size_t", "n")] + [
        ("const uint8_t *", q) for q in ("g", "h", "y1", "y2", "r1", "r2", "ctx_bytes")] + [
        ("const uint64_t *", "ctx_off"), ("const uint8_t *", "ctx_present"), ("uint8_t *", "c_out")]


def test_header_constant_and_comment():
    src = _header()
    m = re.search(r"^#define\s+CPZ_STATUS_BAD_GENERATOR\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) == _native.STATUS_BAD_GENERATOR == cp.STATUS_BAD_GENERATOR == 6
    assert "STATUS_BAD_GENERATOR" in cp.__all__
    end = src.index("int %s(" % HOST)
    comment = src[src.rindex("/*", 0, end):end]
    flat = " ".join(comment.replace("*", " ").split())
    for phrase in ("does not synchronise", "Status 6 wins over every other status", "No cache is touched",
                   "the chunk bound is half of it", "do not return CPZ_EGENERATOR", "CPZ_PAIRS_BULK_MAX_PROOFS",
                   "cpz_ctx_fallback_stats is left alone", "no stage 7 or stage 13 is recorded",
                   "profiles/each_gh_ab.json", "Rows may repeat", "returns synchronised"):
        assert phrase in flat, phrase
    assert "@" not in comment                           # every figure is filled in


def test_prototypes_match_the_header():
    class Recorder:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            return self.__dict__["fns"].setdefault(name, types.SimpleNamespace())

    rec = Recorder()
    _native._declare(rec)
    for name in (HOST, DEVICE, CHAL):
        assert name in _native.EXPORTED
        fn = rec.fns[name]
        assert fn.restype is ctypes.c_int
        assert fn.argtypes == [CTYPES[t] for t, _ in _params(name)], (name, fn.argtypes)


def test_built_library_exports_the_entry_points_at_abi_5():
    assert _native.ABI_VERSION == 5
    assert re.search(r"^#define\s+CPZ_ABI_VERSION\s+5\b", _header(), re.M)
    assert os.path.exists(_native.LIB_PATH), "build() leaves the library in the tree"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in (HOST, DEVICE, CHAL):
        assert hasattr(lib, name), name
    assert lib.cpz_abi_version() == 5


def test_rust_declarations():
    with open(os.path.join(ROOT, "rust", "chaum-pedersen-gpu-sys", "src", "lib.rs")) as f:
        src = f.read()
    assert re.search(r"pub const CPZ_STATUS_BAD_GENERATOR: u8 = 6;", src)
    for name in (HOST, DEVICE, CHAL):
        m = re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % name, src)
        assert m, name
        names = [p.split(":")[0].strip() for p in m.group(1).split(",")]
        assert names == [n for _, n in _params(name)]


def test_status_6_is_invalid_generators():
    err = cp.VerifyResult(6).error()
    assert isinstance(err, cp.InvalidParams) and err.args == ("Invalid generators",)
    assert sorted(cp._STATUS_ERR) == [1, 2, 3, 4, 5]
    assert cp.VerifyResult(6).is_err() and "Invalid generators" in repr(cp.VerifyResult(6))


class _NoLibrary:
    """Any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _gpu_without_library():
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = _NoLibrary()
    g._h = None
    return g


N = 6


def _rows(k=7):
    return [np.zeros((N, 32), np.uint8) for _ in range(k)]


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("bad", [np.zeros((N - 1, 32), np.uint8), np.zeros((N, 31), np.uint8),
                                 np.zeros((N + 1, 32), np.uint8), np.zeros((2, N // 2, 32), np.uint8),
                                 np.zeros(32 * N + 1, np.uint8), "no rows"])
def test_bad_row_shapes_are_rejected_before_the_library_is_called(which, bad):
    rows = _rows()
    rows[which] = bad                                   # (y1 sets n: as y1, the bad row makes the others the odd ones)
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_gh(*rows)
    if which < 6:
        with pytest.raises(cp.InvalidParams):
            _gpu_without_library().challenges_gh(*rows[:6])


def test_empty_and_oversized_calls_are_rejected_before_the_library_is_called():
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_gh(*[np.zeros((0, 32), np.uint8) for _ in range(7)])
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_gh(*_rows(), contexts=[None] * (N - 1))

    class Huge:                                          # len() alone is looked at before anything is copied
        def __len__(self):
            return _native.PAIRS_BULK_MAX_PROOFS + 1

    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_gh(*([np.zeros((1, 32), np.uint8)] * 2 + [Huge()] + _rows(4)))


class _FakeTensor:
    def __init__(self, nbytes, dtype="torch.uint8", cuda=True, contiguous=True, ptr=256):
        self.dtype, self.is_cuda, self._n, self._c, self._p = dtype, cuda, nbytes, contiguous, ptr

    def numel(self):
        return self._n

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return self._p


@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("bad", [_FakeTensor(32 * (N - 1)), _FakeTensor(32 * N, dtype="torch.int32"),
                                 _FakeTensor(32 * N, cuda=False), _FakeTensor(32 * N, contiguous=False),
                                 _FakeTensor(32 * N + 1), _FakeTensor(0), np.zeros((N, 32), np.uint8)])
def test_bad_device_tensors_are_rejected_before_the_library_is_called(which, bad):
    args = [_FakeTensor(32 * N) for _ in range(7)] + [_FakeTensor(N)]
    args[which] = bad
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_gh_device(*args, stream=0)


@pytest.mark.parametrize("eq_only", [True, False])
def test_good_arguments_reach_the_library(eq_only):
    seen = {}

    class Lib:
        def cpz_verify_each_gh(self, h, flags, n, g, hh, y1, y2, r1, r2, s, cb, co, cpres, status):
            seen.update(flags=flags, n=n, g=ctypes.string_at(g, 32 * n), h=ctypes.string_at(hh, 32 * n),
                        s=ctypes.string_at(s, 32 * n), present=ctypes.string_at(cpres, n), ctx=ctypes.string_at(cb, 3))
            ctypes.memmove(status, bytes([0, 1, 2, 3, 4, 6]), n)
            return 0

        def cpz_challenges_gh(self, h, n, g, hh, y1, y2, r1, r2, cb, co, cpres, c_out):
            seen.update(chal_n=n, chal_ctx=(cb, co, cpres))
            ctypes.memset(c_out, 7, 32 * n)
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    rows = [np.full((N, 32), k + 1, np.uint8) for k in range(7)]
    st = g.verify_each_gh(*rows, contexts=[None, b"abc", None, None, None, b""], equations_only=eq_only)
    assert seen == {"flags": _native.CALL_EQUATIONS_ONLY if eq_only else 0, "n": N, "g": b"\x01" * 32 * N,
                    "h": b"\x02" * 32 * N, "s": b"\x07" * 32 * N, "present": bytes([0, 1, 0, 0, 0, 1]), "ctx": b"abc"}
    assert st.dtype == np.uint8 and st.tolist() == [0, 1, 2, 3, 4, 6]
    c = g.challenges_gh(*rows[:6])
    assert seen["chal_n"] == N and seen["chal_ctx"] == (None, None, None) and c.shape == (N, 32) and (c == 7).all()
