"""cpz_verify_each_gh without a GPU: the parts csrc/each_gh.h shares with the kernels, on the CPU
build of the device headers (tests/native/hostlib_gh.cpp, under CPZ_BOUNDS_CHECK) -- the entry's
challenge from the one snapshot no pair enters, against the C oracle's challenge under non-default
pairs for the four context shapes; the generator verdict on the five bad-generator kinds and on good
rows; and the addressing of a quad's four tables in a launch's scratch."""
import ctypes
import hashlib

import pytest

import pyoracle as O


@pytest.fixture(scope="module")
def hostlib():
    import build_native
    lib = ctypes.CDLL(build_native.build_hosttest())
    lib.cpzt_gh_challenge.restype = None
    lib.cpzt_gh_challenge.argtypes = [ctypes.c_char_p] * 7 + [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32]
    lib.cpzt_gh_generators_bad.restype = ctypes.c_int
    lib.cpzt_gh_generators_bad.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.cpzt_gh_quad_tab.restype = ctypes.c_longlong
    lib.cpzt_gh_quad_tab.argtypes = [ctypes.c_longlong, ctypes.c_int]
    lib.cpzt_gh_table_ints.restype = ctypes.c_int
    lib.cpzt_gh_proof_scratch.restype = ctypes.c_longlong
    return lib


def _point(tag):
    return O.ristretto_encode(O.pt_mul(O.BASEPOINT, O.scalar_wide(hashlib.sha512(tag).digest())))


BAD_POINT = bytes.fromhex("01" + "00" * 31)
ZERO = bytes(32)
CONTEXTS = [None, b"", hashlib.sha256(b"ctx").digest(), b"ctx07", bytes(range(200)), b"x" * 167]


@pytest.mark.parametrize("ctx", CONTEXTS, ids=lambda c: "none" if c is None else "len%d" % len(c))
def test_challenge_is_the_oracles_under_the_entrys_own_pair(hostlib, ctx):
    """Absent, empty, 32-byte aligned and odd-length contexts (and two that cross the sponge's rate)."""
    import coracle
    seen = set()
    for k in range(4):
        g, h = _point(b"gh-g-%d" % k), _point(b"gh-h-%d" % k)
        assert g != coracle.DEFAULT_G and h != coracle.DEFAULT_H
        y1, y2, r1, r2 = (_point(b"gh-%s-%d" % (q, k)) for q in (b"y1", b"y2", b"r1", b"r2"))
        out = ctypes.create_string_buffer(32)
        cb = b"" if ctx is None else ctx
        hostlib.cpzt_gh_challenge(out, g, h, y1, y2, r1, r2, 0 if ctx is None else 1, cb, len(cb))
        assert out.raw == coracle.challenge(g, h, y1, y2, r1, r2, ctx), k
        seen.add(out.raw)
    assert len(seen) == 4


def test_challenge_under_the_default_pair(hostlib):
    import coracle
    y1, y2, r1, r2 = (_point(b"gh-d-%s" % q) for q in (b"y1", b"y2", b"r1", b"r2"))
    out = ctypes.create_string_buffer(32)
    hostlib.cpzt_gh_challenge(out, coracle.DEFAULT_G, coracle.DEFAULT_H, y1, y2, r1, r2, 0, b"", 0)
    assert out.raw == coracle.challenge(coracle.DEFAULT_G, coracle.DEFAULT_H, y1, y2, r1, r2, None)


def test_generator_verdict(hostlib):
    assert O.ristretto_decode(BAD_POINT) is None        # the precondition of the two undecodable kinds
    g, h = _point(b"verdict-g"), _point(b"verdict-h")
    bad = {"g undecodable": (BAD_POINT, h), "h undecodable": (g, BAD_POINT), "g identity": (ZERO, h),
           "h identity": (g, ZERO), "g == h": (g, g), "both undecodable": (BAD_POINT, BAD_POINT),
           "both identity": (ZERO, ZERO)}
    for what, (a, b) in bad.items():
        assert hostlib.cpzt_gh_generators_bad(a, b) == 1, what
    import coracle
    good = [(g, h), (h, g), (coracle.DEFAULT_G, coracle.DEFAULT_H), (g, coracle.DEFAULT_H)]
    good += [(_point(b"v-%d" % k), _point(b"w-%d" % k)) for k in range(8)]
    # one bit apart in the last word, and in the first: equal only if every word is compared
    for a, b in good:
        assert hostlib.cpzt_gh_generators_bad(a, b) == 0
    near = bytearray(g)
    near[31] ^= 0x40
    if O.ristretto_decode(bytes(near)) is not None:
        assert hostlib.cpzt_gh_generators_bad(g, bytes(near)) == 0


def test_table_addressing(hostlib):
    """Four tables of 9 x 40 ints per quad, consecutive and disjoint over a launch; a proof (two quads)
    takes twice the eight-lane kernel's two-table scratch, so a slab holds half as many proofs."""
    ints = hostlib.cpzt_gh_table_ints()
    assert ints == 9 * 40
    per_proof = hostlib.cpzt_gh_proof_scratch()
    assert per_proof == 2 * 4 * ints * 4 == 2 * (2 * 2 * ints * 4)
    proofs = 8192                                        # one launch on a 256-CU part: half of 16384
    nxt = 0
    for slot in list(range(0, 70)) + list(range(2 * proofs - 70, 2 * proofs)):
        if slot == 2 * proofs - 70:
            nxt = slot * 4 * ints
        for t in range(4):
            assert hostlib.cpzt_gh_quad_tab(slot, t) == nxt
            nxt += ints
    assert nxt * 4 == proofs * per_proof == 16384 * (per_proof // 2)      # the slab of 16384 two-table proofs
    # 2^21 quads (2^20 proofs in one launch would be) still index in 64 bits
    assert hostlib.cpzt_gh_quad_tab(2 ** 21, 3) == (2 ** 21 * 4 + 3) * ints
