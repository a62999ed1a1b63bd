"""Host-side checks of the mixed-pair call (Gpu.verify_each_pairs): the index array is
validated before the library is called, and the binding declares both entry points."""
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
        _gpu_without_library().verify_each_pairs(PAIRS, idx, *ROWS)


def test_good_pair_idx_reaches_the_library_as_uint32():
    seen = {}

    class Lib:
        def cpz_verify_each_pairs_ex(self, h, flags, npairs, gh, n, idx, *rest):
            seen.update(flags=flags, npairs=npairs, n=n,
                        idx=np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint32 * n).from_address(idx)).tolist())
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    g.verify_each_pairs(PAIRS, np.array([2, 0, 1, 2], np.int64), *ROWS, equations_only=True)
    assert seen == {"flags": _native.CALL_EQUATIONS_ONLY, "npairs": 3, "n": 4, "idx": [2, 0, 1, 2]}


def test_binding_exports_both_entry_points():
    assert "cpz_verify_each_pairs" in _native.EXPORTED and "cpz_verify_each_pairs_ex" in _native.EXPORTED
    assert (_native.PAIRS_MAX, _native.PAIRS_MAX_PROOFS) == (64, 2048)
    assert _native.ABI_VERSION == 5
