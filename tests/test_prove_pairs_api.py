"""Host-side checks of the mixed-pair prover's bindings (Gpu.prove_pairs and
Gpu.prove_pairs_device): the index array is validated before the library is called, and the
binding declares the two entry points and the bound."""
import os
import re

import numpy as np
import pytest

import chaum_pedersen as cp
from chaum_pedersen import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoLibrary:
    """Any call into the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _gpu_without_library():
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = _NoLibrary()
    g._h = None
    return g


X = [1, 2, 3, 4]
K = [5, 6, 7, 8]
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
        _gpu_without_library().prove_pairs(PAIRS, idx, X, K)


def test_good_pair_idx_reaches_the_library_as_uint32():
    seen = {}

    class Lib:
        def cpz_prove_pairs(self, h, npairs, gh, n, idx, x, k, *rest):
            u32 = np.ctypeslib.ctypes.c_uint32
            u8 = np.ctypeslib.ctypes.c_uint8
            seen.update(npairs=npairs, n=n, rest=len(rest),
                        idx=np.ctypeslib.as_array((u32 * n).from_address(idx)).tolist(),
                        x=bytes((u8 * (32 * n)).from_address(x)), k0=bytes((u8 * 32).from_address(k)))
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    out = g.prove_pairs(PAIRS, np.array([2, 0, 1, 2], np.int64), X, K, contexts=[None, b"a", b"", None])
    assert seen == {"npairs": 3, "n": 4, "rest": 8, "idx": [2, 0, 1, 2],
                    "x": b"".join(v.to_bytes(32, "little") for v in X), "k0": (5).to_bytes(32, "little")}
    assert sorted(out) == ["r1", "r2", "s", "y1", "y2"] and all(v.shape == (4, 32) for v in out.values())


def test_binding_exports_the_two_entry_points_and_the_bound():
    for name in ("cpz_prove_pairs", "cpz_prove_pairs_device"):
        assert name in _native.EXPORTED, name
    assert _native.PROVE_PAIRS_MAX_PROOFS == 1 << 20
    with open(os.path.join(ROOT, "include", "cpz.h")) as f:
        header = f.read()
    m = re.search(r"^#define\s+CPZ_PROVE_PAIRS_MAX_PROOFS\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == 1 << 20
    for name in ("cpz_prove_pairs", "cpz_prove_pairs_device"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert _native.ABI_VERSION == 5 and re.search(r"^#define\s+CPZ_ABI_VERSION\s+5\b", header, re.M)


class _Tensor:
    """What the device method looks at in a torch tensor (the suite's CPU half needs no torch)."""

    def __init__(self, shape, dtype, is_cuda=True, contiguous=True):
        self.shape, self.dtype, self.is_cuda, self._contiguous = tuple(shape), dtype, is_cuda, contiguous
        self.device = "cuda:0" if is_cuda else "cpu"

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return 0x1000


def test_device_method_refuses_a_bad_pair_idx_before_the_library_is_called():
    rows = [_Tensor((4, 32), "torch.uint8") for _ in range(7)]
    g = _gpu_without_library()
    for bad in (
        np.array([0, 1, 2, 0], np.uint32),                    # a host array
        [0, 1, 2, 0],                                         # a list
        _Tensor((4,), "torch.int64"),                         # wrong dtype
        _Tensor((4,), "torch.float32"),                       # wrong dtype
        _Tensor((3,), "torch.int32"),                         # too short
        _Tensor((5,), "torch.int32"),                         # too long
        _Tensor((2, 2), "torch.int32"),                       # not one-dimensional
        _Tensor((4,), "torch.int32", contiguous=False),       # strided
        _Tensor((4,), "torch.int32", is_cuda=False),          # right shape and dtype, but a host tensor
    ):
        with pytest.raises(cp.InvalidParams):
            g.prove_pairs_device(PAIRS, bad, *rows)


def test_device_method_passes_a_good_pair_idx_on():
    seen = {}

    class Lib:
        def cpz_prove_pairs_device(self, h, npairs, gh, n, idx, *rest):
            seen.update(npairs=npairs, n=n, idx=idx, rest=len(rest), stream=rest[-1])
            return 0

    g = _gpu_without_library()
    g._lib = Lib()
    rows = [_Tensor((4, 32), "torch.uint8") for _ in range(7)]
    for dtype in ("torch.int32", "torch.uint32"):
        g.prove_pairs_device(PAIRS, _Tensor((4,), dtype), *rows, stream=7)
        assert seen == {"npairs": 3, "n": 4, "idx": 0x1000, "rest": 11, "stream": 7}
