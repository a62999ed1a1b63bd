"""Host-side checks of the mixed-pair batch check (Gpu.verify_batch_pairs): the index array is
validated before the library is called, good indices reach cpz_verify_batch_pairs_ex as uint32
with the call's flags, and the binding and the built library carry both entry points."""
import ctypes
import os

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native


class _NoLibrary:
    """Any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _gpu_without_library():
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = _NoLibrary()
    g._h = None
    return g


ROWS = [np.zeros((4, 32), np.uint8) for _ in range(5)]
PAIRS = [cp.Parameters(bytes([1 + i]) * 32, bytes([9 + i]) * 32) for i in range(3)]
SEED = bytes(range(32))


@pytest.mark.parametrize("idx", [
    [0, 1, 2],                            # too short
    [0, 1, 2, 0, 1],                      # too long
    [[0, 1], [2, 0]],                     # not one-dimensional
    [0, 1, 3, 0],                         # 3 is not below the 3 pairs
    [0, -1, 2, 0],                        # negative
    np.array([0, 1, 2 ** 32, 0], np.int64),   # would wrap to 0 as uint32
    [0.0, 1.0, 2.0, 0.0],                 # not integers
    [True, False, True, False],           # not integers
])
def test_bad_pair_idx_is_rejected_before_the_library_is_called(idx):
    with pytest.raises(cp.InvalidParams):
        _gpu_without_library().verify_batch_pairs(PAIRS, idx, *ROWS, SEED)


@pytest.mark.parametrize("statuses", [True, False])
def test_good_pair_idx_reaches_the_library_as_uint32_with_the_flags(statuses):
    seen = {}

    class Lib:
        def cpz_verify_batch_pairs_ex(self, h, flags, npairs, gh, n, idx, y1, y2, r1, r2, s, cb, co, cpres, seed,
                                      first_index, partial, ok, status):
            seen.update(flags=flags, npairs=npairs, n=n, seed=seed, first_index=first_index, status=status is not None,
                        gh=ctypes.string_at(gh, 64 * npairs),
                        idx=np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(idx)).tolist())
            ctypes.memmove(partial, bytes([7]) * 32, 32)
            ok._obj.value = 1
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    partial, ok, st = g.verify_batch_pairs(PAIRS, np.array([2, 0, 1, 2], np.int64), *ROWS, SEED, first_index=77,
                                           statuses=statuses, equations_only=True)
    assert seen == {"flags": _native.CALL_EQUATIONS_ONLY, "npairs": 3, "n": 4, "idx": [2, 0, 1, 2], "seed": SEED,
                    "first_index": 77, "status": statuses, "gh": b"".join(p.g + p.h for p in PAIRS)}
    assert partial == bytes([7]) * 32 and ok is True
    assert (st is not None) == statuses and (st is None or st.shape == (4,))


def test_binding_declares_both_entry_points_and_the_bound():
    assert "cpz_verify_batch_pairs" in _native.EXPORTED and "cpz_verify_batch_pairs_ex" in _native.EXPORTED
    assert _native.BATCH_PAIRS_MAX_PROOFS == 1 << 20
    assert (_native.PAIRS_MAX, _native.PAIRS_MAX_PROOFS) == (64, 2048)
    assert _native.ABI_VERSION == 5


def test_built_library_exports_both_entry_points():
    assert os.path.exists(_native.LIB_PATH), "build() leaves the library in the tree"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("cpz_verify_batch_pairs", "cpz_verify_batch_pairs_ex"):
        assert hasattr(lib, name), name
    assert lib.cpz_abi_version() == 5


def test_header_bound_matches_the_binding():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpz.h")).read()
    assert "#define CPZ_BATCH_PAIRS_MAX_PROOFS %d" % _native.BATCH_PAIRS_MAX_PROOFS in src
