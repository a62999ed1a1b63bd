"""Host-side checks of cpz_verify_each_pairs_many / Gpu.verify_each_pairs_many: the header declares
the entry point and its bound and says what the call does above CPZ_PAIRS_MAX pairs, the ctypes
prototype follows the header's, the ABI version stays 5, the built library exports the symbol, the
wrapper checks its pairs and indices before the library is called, and BatchVerifier.verify sends
more than PAIRS_MAX per-proof groups out as one such call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cpz_verify_each_pairs_many"
SIBLING = "cpz_verify_each_pairs_bulk_ex"
CTYPES = {"cpz_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
          "const uint8_t *": ctypes.c_void_p, "const uint32_t *": ctypes.c_void_p, "const uint64_t *": ctypes.c_void_p,
          "uint8_t *": ctypes.c_void_p}


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


def test_header_declares_the_entry_point_like_its_sibling():
    many, bulk = _params(NAME), _params(SIBLING)
    assert many == bulk
    assert [n for _, n in many] == ["ctx", "flags", "npairs", "pairs", "n", "pair_idx", "y1", "y2", "r1", "r2", "s",
                                    "ctx_bytes", "ctx_off", "ctx_present", "status_out"]


def test_header_constant_and_comment():
    src = _header()
    m = re.search(r"^#define\s+CPZ_EACH_PAIRS_MANY_MAX\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) == _native.EACH_PAIRS_MANY_MAX == 4096
    # the comment that precedes the declaration
    end = src.index("#define CPZ_EACH_PAIRS_MANY_MAX")
    comment = src[src.rindex("/*", 0, end):end]
    flat = " ".join(comment.replace("*", " ").split())
    for phrase in ("CPZ_EACH_PAIRS_MANY_MAX", "npairs <= CPZ_PAIRS_MAX is cpz_verify_each_pairs_bulk_ex itself",
                   "CPZ_EACH_MANY_FORWARD=0", "Host buffers only", "one stage-13 span whose launch count is npairs",
                   "builds no 128-entry set", "5,760 bytes per pair", "cpz_ctx_pairs_resident answers the same",
                   "status_out is not written on an error"):
        assert phrase in flat, phrase
    # the sibling keeps its own bound, and stage 13's sentence knows the new span
    assert "npairs > CPZ_PAIRS_MAX" in src
    stages = " ".join(src[src.index("Per-kernel timing"):src.index("#define CPZ_NUM_STAGES")].replace("*", " ").split())
    assert "cpz_verify_each_pairs_many" in stages and "launch count is npairs" in stages
    assert "at most 16384 proofs on a pair" not in stages      # the bound depends on the device's CUs
    assert re.search(r"^#define\s+CPZ_NUM_STAGES\s+16\b", src, re.M)


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
    assert fn.argtypes == rec.fns[SIBLING].argtypes


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
        _gpu_without_library().verify_each_pairs_many(PAIRS, idx, *ROWS)


@pytest.mark.parametrize("pairs", [PAIRS[0], PAIRS[:3] + [b"\x01" * 64], b"\x01" * 64 * NP])
def test_pairs_that_are_not_parameters_are_rejected_before_the_library_is_called(pairs):
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_each_pairs_many(pairs, [0] * N, *ROWS)


def test_row_shapes_are_checked_before_the_library_is_called():
    rows = [r.copy() for r in ROWS]
    rows[3] = np.zeros((N - 1, 32), np.uint8)
    with pytest.raises(ValueError):   # as every wrapper's row check reports it
        _gpu_without_library().verify_each_pairs_many(PAIRS, [0] * N, *rows)


@pytest.mark.parametrize("eq_only", [True, False])
def test_good_arguments_reach_the_library(eq_only):
    seen = {}

    class Lib:
        def cpz_verify_each_pairs_many(self, h, flags, npairs, gh, n, idx, y1, y2, r1, r2, s, cb, co, cpres, status):
            seen.update(flags=flags, npairs=npairs, n=n, gh=ctypes.string_at(gh, 64 * npairs),
                        idx=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(idx)).tolist(),
                        present=ctypes.string_at(cpres, n), ctx=ctypes.string_at(cb, 3))
            ctypes.memmove(status, bytes([0, 1, 2, 3, 4, 5]), n)
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    st = g.verify_each_pairs_many(PAIRS, np.array([69, 0, 1, 2, 69, 5], np.int64), *ROWS,
                                  contexts=[None, b"abc", None, None, None, b""], equations_only=eq_only)
    assert seen == {"flags": _native.CALL_EQUATIONS_ONLY if eq_only else 0, "npairs": NP, "n": N,
                    "idx": [69, 0, 1, 2, 69, 5], "gh": b"".join(p.g + p.h for p in PAIRS),
                    "present": bytes([0, 1, 0, 0, 0, 1]), "ctx": b"abc"}
    assert st.dtype == np.uint8 and st.tolist() == [0, 1, 2, 3, 4, 5]


# ---- BatchVerifier.verify ---------------------------------------------------------------------------

class _RecordingGpu:
    """Stands in for Gpu: records the per-proof calls and answers every entry with status 0, but
    for the entries whose s is all 0x01 bytes, which get status 1."""

    def __init__(self):
        self.calls = []

    def _answer(self, s):
        return np.array([1 if bytes(row) == b"\x01" * 32 else 0 for row in np.asarray(s)], np.uint8)

    def verify_each(self, y1, y2, r1, r2, s, contexts=None, params=None, equations_only=False):
        self.calls.append(("verify_each", None, None, np.asarray(y1).copy(), contexts, equations_only))
        return self._answer(s)

    def verify_each_pairs(self, pairs, pair_idx, y1, y2, r1, r2, s, contexts=None, equations_only=False):
        self.calls.append(("verify_each_pairs", list(pairs), np.asarray(pair_idx).tolist(), np.asarray(y1).copy(),
                           contexts, equations_only))
        return self._answer(s)

    def verify_each_pairs_many(self, pairs, pair_idx, y1, y2, r1, r2, s, contexts=None, equations_only=False):
        self.calls.append(("verify_each_pairs_many", list(pairs), np.asarray(pair_idx).tolist(), np.asarray(y1).copy(),
                           contexts, equations_only))
        return self._answer(s)

    def decode_points(self, points):      # Statement::validate: every statement decodes
        return np.ones(len(points), np.uint8), None

    def verify_batch(self, *a, **k):
        raise AssertionError("no group reaches the RLC threshold")


def _params_of(k):
    return cp.Parameters(bytes([k + 1]) * 32, bytes([k + 1, 7] * 16))


def _batch(gpu, n, npairs, forged=()):
    """Entry i under Parameters i % npairs, y1 = i as 32 bytes; forged entries carry s = 0x01 * 32."""
    b = cp.BatchVerifier(gpu)
    for i in range(n):
        tag = i.to_bytes(32, "little")
        s = b"\x01" * 32 if i in forged else b"\x02" * 32
        b.add_with_context(_params_of(i % npairs), cp.Statement(tag, tag), cp.Proof(tag, tag, s),
                           None if i % 3 == 0 else b"c%d" % i)
    return b


def test_batch_verifier_sends_65_groups_as_one_many_call():
    rec = _RecordingGpu()
    res = _batch(rec, 130, 65, forged=(0, 64, 65, 129)).verify()
    assert len(rec.calls) == 1
    name, pairs, idx, y1, ctxs, eq_only = rec.calls[0]
    assert name == "verify_each_pairs_many" and eq_only is True
    assert pairs == [_params_of(k) for k in range(65)]              # order of first appearance
    assert idx == [i % 65 for i in range(130)]                      # entry i under its own Parameters
    assert [bytes(r) for r in y1] == [i.to_bytes(32, "little") for i in range(130)]     # batch order
    assert ctxs == [None if i % 3 == 0 else b"c%d" % i for i in range(130)]
    assert [r.status for r in res] == [1 if i in (0, 64, 65, 129) else 0 for i in range(130)]


def test_batch_verifier_keeps_64_groups_on_the_resident_call():
    rec = _RecordingGpu()
    res = _batch(rec, 128, 64, forged=(5,)).verify()
    assert [c[0] for c in rec.calls] == ["verify_each_pairs"]
    name, pairs, idx, y1, ctxs, eq_only = rec.calls[0]
    assert pairs == [_params_of(k) for k in range(64)] and idx == [i % 64 for i in range(128)] and eq_only is True
    assert [bytes(r) for r in y1] == [i.to_bytes(32, "little") for i in range(128)]
    assert [r.status for r in res] == [1 if i == 5 else 0 for i in range(128)]


def test_batch_verifier_leaves_the_rng_draws_alone():
    """One 64-byte draw per entry whatever entry point the groups take."""
    class Rng:
        def __init__(self):
            self.draws = []

        def randbytes(self, k):
            self.draws.append(k)
            return bytes(k)

    rng = Rng()
    _batch(_RecordingGpu(), 130, 65).verify(rng=rng)
    assert rng.draws == [64] * 130
