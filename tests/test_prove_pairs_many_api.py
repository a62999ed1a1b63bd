"""Host-side checks of cpz_prove_pairs_many[_device] / Gpu.prove_pairs_many[_device]: the header
declares the entry points like cpz_prove_pairs[_device] and says what the call does above
CPZ_PAIRS_MAX pairs, the bound agrees between cpz.h, _native.py and the Rust crate, the ctypes
prototypes follow the header's, the ABI version stays 5, the built library exports the symbols, the
wrapper checks its arguments before the library is called -- and, on the host build of the device
headers, the digits k_prove_points_micro walks (sc_recode_radix16 of the scalar mod l) are in range,
have the scalar's value, lose no carry between digit 31 (the last on B) and digit 32 (the first on
2^128 B) and leave none out of the top."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native
from prove_many_cases import EDGES, L, recode_radix16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cpz_prove_pairs_many": "cpz_prove_pairs", "cpz_prove_pairs_many_device": "cpz_prove_pairs_device"}
CTYPES = {"cpz_ctx *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "const uint8_t *": ctypes.c_void_p,
          "const uint32_t *": ctypes.c_void_p, "const uint64_t *": ctypes.c_void_p, "uint8_t *": ctypes.c_void_p,
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


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_declares_the_entry_point_like_its_sibling(name):
    assert _params(name) == _params(NAMES[name])
    assert [n for _, n in _params("cpz_prove_pairs_many")] == [
        "ctx", "npairs", "pairs", "n", "pair_idx", "x", "k", "ctx_bytes", "ctx_off", "ctx_present", "y1", "y2", "r1",
        "r2", "s"]


def test_the_bound_agrees_between_header_python_and_rust():
    src = _header()
    m = re.search(r"^#define\s+CPZ_PROVE_PAIRS_MANY_MAX\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) == _native.PROVE_PAIRS_MANY_MAX == 4096
    with open(os.path.join(ROOT, "rust", "chaum-pedersen-gpu-sys", "src", "lib.rs")) as f:
        rust = f.read()
    r = re.search(r"^pub const CPZ_PROVE_PAIRS_MANY_MAX: usize = (\d+);", rust, re.M)
    assert r and int(r.group(1)) == 4096
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, rust), name
    # the siblings keep their own bounds
    assert _native.PAIRS_MAX == 64 and _native.PROVE_PAIRS_MAX_PROOFS == 1 << 20
    assert _native.PROVE_PAIRS_MANY_MAX == _native.EACH_PAIRS_MANY_MAX == _native.BATCH_PAIRS_MANY_MAX


def test_header_comment_and_stage_sentences():
    src = _header()
    end = src.index("#define CPZ_PROVE_PAIRS_MANY_MAX")
    comment = src[src.rindex("/*", 0, end):end]
    flat = " ".join(comment.replace("*", " ").split())
    for phrase in ("CPZ_PROVE_PAIRS_MANY_MAX", "npairs <= CPZ_PAIRS_MAX is cpz_prove_pairs[_device] itself",
                   "CPZ_PROVE_MANY_FORWARD=0", "one stage-13 span whose launch count is npairs",
                   "builds no 128-entry set", "5,760 bytes per pair", "cpz_ctx_pairs_resident answers the same",
                   "leaves cpz_ctx_fallback_stats alone", "stage 6", "No output is written on an error",
                   "profiles/prove_pairs_many_ab.json"):
        assert phrase in flat, phrase
    stages = " ".join(src[src.index("Per-kernel timing"):src.index("#define CPZ_NUM_STAGES")].replace("*", " ").split())
    assert "cpz_verify_each_pairs_many and cpz_prove_pairs_many above CPZ_PAIRS_MAX pairs" in stages
    assert "cpz_prove_pairs_many's point kernel" in stages
    assert re.search(r"^#define\s+CPZ_NUM_STAGES\s+16\b", src, re.M)


def test_prototypes_match_the_header():
    class Recorder:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            return self.__dict__["fns"].setdefault(name, types.SimpleNamespace())

    rec = Recorder()
    _native._declare(rec)
    for name, sibling in NAMES.items():
        assert name in _native.EXPORTED
        fn = rec.fns[name]
        assert fn.restype is ctypes.c_int
        assert fn.argtypes == [CTYPES[t] for t, _ in _params(name)], (name, fn.argtypes)
        assert fn.argtypes == rec.fns[sibling].argtypes


def test_abi_version_is_still_5():
    assert _native.ABI_VERSION == 5
    assert re.search(r"^#define\s+CPZ_ABI_VERSION\s+5\b", _header(), re.M)


def test_built_library_exports_the_entry_points():
    assert os.path.exists(_native.LIB_PATH), "build() leaves the library in the tree"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.cpz_abi_version() == 5


# ---- the digits of the walk, on the host build of the device headers ----------------------------------

@pytest.fixture(scope="module")
def hostlib():
    import build_native
    lib = ctypes.CDLL(build_native.build_hosttest())
    lib.cpzt_prove_many_digits.restype = None
    lib.cpzt_prove_many_digits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    return lib


def _digits(lib, raw):
    dg = (ctypes.c_int8 * 64)()
    red = ctypes.create_string_buffer(32)
    lib.cpzt_prove_many_digits(dg, red, raw)
    return list(dg), int.from_bytes(red.raw, "little")


# adding 8 to every nibble with the carries passed on is adding 0x88..88: the carry out of digit 31
EIGHTS = int.from_bytes(b"\x88" * 16, "little")


def test_digits_of_the_edges_and_of_random_scalars(hostlib):
    rng = np.random.default_rng(20262)
    cases = list(EDGES) + [("random %d" % i, (int.from_bytes(rng.bytes(64), "little") % L).to_bytes(32, "little"))
                           for i in range(200)]
    assert len(EDGES) == 14
    carried = 0
    for name, raw in cases:
        dg, red = _digits(hostlib, raw)
        v = int.from_bytes(raw, "little") % L
        assert red == v, name                                          # reduced as prove_scalar reduces it
        assert len(dg) == 64 and all(-8 <= d <= 7 for d in dg), (name, dg)
        assert sum(d << (4 * i) for i, d in enumerate(dg)) == v, name
        model, carry_out = recode_radix16(v)
        assert dg == model and carry_out == 0, name
        assert 0 <= dg[63] <= 2, (name, dg[63])                        # v < l < 2^252 + 2^125: nothing leaves the top
        # the two halves the walk puts on B and on 2^128 B: the low one is v mod 2^128 less the carry
        # that digit 32 holds, so that lo + 2^128 hi is v
        lo = sum(d << (4 * i) for i, d in enumerate(dg[:32]))
        hi = sum(d << (4 * i) for i, d in enumerate(dg[32:]))
        c31 = ((v & ((1 << 128) - 1)) + EIGHTS) >> 128                # the carry chain of the low 32 nibbles
        assert lo == (v & ((1 << 128) - 1)) - (c31 << 128) and hi == (v >> 128) + c31, name
        assert lo + (hi << 128) == v
        carried += c31
    assert carried > 50                                               # both sides of the carry were seen
    by_name = dict(cases)
    assert _digits(hostlib, by_name["2^128-1"])[0] == [-1] + [0] * 31 + [1] + [0] * 31
    assert _digits(hostlib, by_name["2^128"])[0] == [0] * 32 + [1] + [0] * 31
    assert _digits(hostlib, by_name["2^128+8"])[0] == [-8, 1] + [0] * 30 + [1] + [0] * 31
    assert _digits(hostlib, by_name["8"])[0] == [-8, 1] + [0] * 62
    assert _digits(hostlib, by_name["7"])[0] == [7] + [0] * 63
    assert _digits(hostlib, by_name["2^252"])[0] == [0] * 63 + [1]
    assert _digits(hostlib, by_name["2^124"])[0] == [0] * 31 + [1] + [0] * 32
    assert _digits(hostlib, by_name["0"])[0] == [0] * 64
    assert _digits(hostlib, by_name["2^256-1 unreduced"])[1] == (2**256 - 1) % L


# ---- the wrapper's checks ----------------------------------------------------------------------------------

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
XS = np.zeros((N, 32), np.uint8)
PAIRS = [cp.Parameters(bytes([1 + i]) * 32, bytes([101 + i]) * 32) for i in range(NP)]


@pytest.mark.parametrize("idx", [
    [0, 1, 2, 3, 69],                          # too short
    [0, 1, 2, 3, 4, 5, 6],                     # too long
    [[0, 1, 2], [3, 4, 5]],                    # not one-dimensional
    [0, 1, 70, 0, 1, 2],                       # 70 is not below the 70 pairs
    [0, -1, 2, 0, 1, 2],                       # negative
    np.array([0, 1, 2 ** 32, 0, 1, 2], np.int64),   # would wrap to 0 as uint32
    [0.0, 1.0, 2.0, 0.0, 1.0, 2.0],            # not integers
])
def test_bad_pair_idx_is_rejected_before_the_library_is_called(idx):
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().prove_pairs_many(PAIRS, idx, XS, XS)


@pytest.mark.parametrize("pairs", [PAIRS[0], PAIRS[:3] + [b"\x01" * 64], b"\x01" * 64 * NP])
def test_pairs_that_are_not_parameters_are_rejected_before_the_library_is_called(pairs):
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().prove_pairs_many(pairs, [0] * N, XS, XS)
    with pytest.raises(cp.InvalidParams):      # the device form: a host index array is refused first
        _gpu_without_library().prove_pairs_many_device(PAIRS, np.zeros(N, np.int32), XS, XS, XS, XS, XS, XS, XS)


def test_contexts_of_another_length_are_rejected_before_the_library_is_called():
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().prove_pairs_many(PAIRS, [0] * N, XS, XS, contexts=[b"a"] * (N - 1))


def test_good_arguments_reach_the_library():
    seen = {}

    class Lib:
        def cpz_prove_pairs_many(self, h, npairs, gh, n, idx, x, k, cb, co, cpres, y1, y2, r1, r2, s):
            seen.update(npairs=npairs, n=n, gh=ctypes.string_at(gh, 64 * npairs),
                        idx=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(idx)).tolist(),
                        x=ctypes.string_at(x, 32 * n), k=ctypes.string_at(k, 32 * n),
                        present=ctypes.string_at(cpres, n), ctx=ctypes.string_at(cb, 3))
            for j, p in enumerate((y1, y2, r1, r2, s)):
                ctypes.memset(p, j + 1, 32 * n)
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    out = g.prove_pairs_many(PAIRS, np.array([69, 0, 1, 2, 69, 5], np.int64), [1, 2, 3, 4, 5, L + 6], [9] * N,
                             contexts=[None, b"abc", None, None, None, b""])
    assert seen == {"npairs": NP, "n": N, "idx": [69, 0, 1, 2, 69, 5], "gh": b"".join(p.g + p.h for p in PAIRS),
                    "x": b"".join(v.to_bytes(32, "little") for v in (1, 2, 3, 4, 5, 6)),
                    "k": (9).to_bytes(32, "little") * N, "present": bytes([0, 1, 0, 0, 0, 1]), "ctx": b"abc"}
    assert [out[q].shape for q in ("y1", "y2", "r1", "r2", "s")] == [(N, 32)] * 5
    assert [int(out[q][0, 0]) for q in ("y1", "y2", "r1", "r2", "s")] == [1, 2, 3, 4, 5]


def test_prove_pairs_keeps_its_own_entry_point():
    """Gpu.prove_pairs still hands its pairs, 70 of them too, to cpz_prove_pairs: the refusal above
    PAIRS_MAX stays the library's."""
    seen = []

    class Lib:
        def cpz_prove_pairs(self, h, npairs, *rest):
            seen.append(npairs)
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    g.prove_pairs(PAIRS, [0] * N, XS, XS)
    assert seen == [NP]
