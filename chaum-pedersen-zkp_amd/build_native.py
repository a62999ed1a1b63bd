"""Build recipes for the in-tree native artefacts (no cmake/ninja needed).

* ``lib/libcpz.so``      -- the product: gfx950 HIP kernels + host runtime + C ABI
                           (hipcc --offload-arch=gfx950).
* ``tests/native/libcpz_hosttest.so`` -- CPU build of the device-library headers with
                           limb-bound assertions, for unit tests only.
* ``tests/native/libcpz_devprobe.so`` -- gfx950 build of the device-only headers (fe16.h,
                           keccak_wave.h, the device arm of the challenge split) behind plain C
                           probes, for the GPU unit tests only; never linked into the product.
* ``tests/native/libcpz_partprobe.so`` -- gfx950 build of csrc/part.hip, included unchanged,
                           behind plain C probes of its kernels (tests/native/partprobe.hip),
                           for the GPU unit tests only; never linked into the product.
* ``tests/native/libcpz_partpairsprobe.so`` -- the same for part.hip's pair mode
                           (tests/native/partpairsprobe.hip), for the GPU unit tests only; never
                           linked into the product.
* ``tests/native/libcpz_partmanyprobe.so`` -- the same for part.hip's many mode (block-local pair
                           slots, tests/native/partmanyprobe.hip), for the GPU unit tests only;
                           never linked into the product.
* ``tests/native/libcpz_msmprobe.so`` -- gfx950 build of csrc/rlc.hip, included unchanged, behind
                           plain C probes of the MSM's sort and reduction kernels
                           (tests/native/msmprobe.hip), for the GPU unit tests only; never linked
                           into the product.
* ``tests/native/libcpz_pairsumprobe.so`` -- the same for rlc.hip's per-pair sum kernels
                           (tests/native/pairsumprobe.hip), for the GPU unit tests only; never
                           linked into the product.
* ``tests/native/libcpz_prepprobe.so`` -- the same for rlc.hip's prepare kernels, the extras' kernels
                           and the device scalar arithmetic (tests/native/prepprobe.hip), for the
                           GPU unit tests only; never linked into the product.
* ``tests/native/libcpz_microprobe.so`` -- gfx950 build of csrc/kernels.hip, included unchanged,
                           behind plain C probes of the small per-pair generator tables
                           (tests/native/microprobe.hip), for the GPU unit tests only; never linked
                           into the product.
* ``oracle/``            -- delegated to oracle/Makefile (the C oracle: CPU baseline and
                           at-scale checker; test infrastructure only).

Each target is rebuilt only when one of its sources is newer than the output.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIBCPZ = os.path.join(LIBDIR, "libcpz.so")
HOSTTEST = os.path.join(ROOT, "tests", "native", "libcpz_hosttest.so")
DEVPROBE = os.path.join(ROOT, "tests", "native", "libcpz_devprobe.so")
PARTPROBE = os.path.join(ROOT, "tests", "native", "libcpz_partprobe.so")
PARTPAIRSPROBE = os.path.join(ROOT, "tests", "native", "libcpz_partpairsprobe.so")
PARTMANYPROBE = os.path.join(ROOT, "tests", "native", "libcpz_partmanyprobe.so")
MSMPROBE = os.path.join(ROOT, "tests", "native", "libcpz_msmprobe.so")
PAIRSUMPROBE = os.path.join(ROOT, "tests", "native", "libcpz_pairsumprobe.so")
PREPPROBE = os.path.join(ROOT, "tests", "native", "libcpz_prepprobe.so")
MICROPROBE = os.path.join(ROOT, "tests", "native", "libcpz_microprobe.so")
ARCH = os.environ.get("CPZ_OFFLOAD_ARCH", "gfx950")


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the gfx950 build needs ROCm")


def _newer(out: str, srcs) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in srcs)


def _headers():
    hdr = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return hdr + [os.path.join(ROOT, "include", "cpz.h")]


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("build step failed: %s\n%s" % (" ".join(cmd), r.stdout[-4000:]))
    return r.stdout


# Per-unit flags: k_verify_wide's single-wave row loops ran 12 % apart with their placement
# (Straus 46.6 against 52.7 us for identical loop code, profiles/r05_wide_align_ab.txt);
# aligned loop heads make that independent of the code before them.
UNIT_FLAGS = {"wide.hip": ["-falign-loops=64"]}


def build_libcpz(force: bool = False, verbose: bool = False, out: str = LIBCPZ, defines=()) -> str:
    """Build the product library.  `out` / `defines` build a tuning variant (e.g.
    CPZ_VERIFY_WAVES=3) elsewhere, for side-by-side measurement with CPZ_LIB=<out>."""
    units = ["kernels.hip", "wide.hip", "rlc.hip", "part.hip", "h2g.hip", "runtime.hip"]
    srcs = [os.path.join(CSRC, u) for u in units] + _headers()
    if not force and not defines and not _newer(out, srcs):
        return out
    objdir = os.path.join(os.path.dirname(out), "obj" if not defines else "obj_" + "_".join(defines).replace("=", ""))
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    common = [hipcc, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", CSRC,
              "-I", os.path.join(ROOT, "include")] + ["-D" + d for d in defines]
    if defines and os.environ.get("CPZ_EXTRA_FLAGS"):  # tuning variants only, never the product build
        common += os.environ["CPZ_EXTRA_FLAGS"].split()

    def compile_one(u):
        obj = os.path.join(objdir, u.replace(".hip", ".o"))
        if force or defines or _newer(obj, [os.path.join(CSRC, u)] + _headers()):
            uf = [] if defines and os.environ.get("CPZ_NO_UNIT_FLAGS") else UNIT_FLAGS.get(u, [])  # variants only
            _run(common + uf + ["-c", os.path.join(CSRC, u), "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        objs = list(ex.map(compile_one, units))
    tmp = out + ".tmp"
    _run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", tmp] + objs)
    os.replace(tmp, out)
    if verbose:
        print("built", out)
    return out


CLOCK_PROBE_LIB = os.path.join(LIBDIR, "timing", "clock_probe.so")


def build_clock_probe(force: bool = False) -> str:
    """Timing-only build with the in-kernel clock probes (csrc/timing_only.h): k_verify_each,
    k_rlc_prepare, k_rlc_bucket stamp their shader clock; tools/time_verify.py reads them.
    Not part of build_all: only the measurement runs load it (CPZ_LIB)."""
    os.makedirs(os.path.dirname(CLOCK_PROBE_LIB), exist_ok=True)
    return build_libcpz(force, out=CLOCK_PROBE_LIB, defines=("CPZ_CLOCK_PROBE", "CPZ_TIMING_ONLY"))


def build_hosttest(force: bool = False, out: str = HOSTTEST, defines=()) -> str:
    """`out` / `defines` build a variant of the device library elsewhere (a switch at 0), so that
    the CPU tests can hold the fallback code to the same checks."""
    srcs = [os.path.join(ROOT, "tests", "native", f) for f in ("hostlib.cpp", "hostlib_joint.cpp", "hostlib_lean.cpp",
                                                              "hostlib_prove.cpp", "hostlib_pairsum.cpp",
                                                              "hostlib_fold.cpp", "hostlib_prove_many.cpp",
                                                              "hostlib_h2g.cpp", "hostlib_gh.cpp")]
    if not force and not _newer(out, srcs + _headers()):
        return out
    cxx = shutil.which("g++") or "g++"
    tmp = out + ".tmp"
    # CPZ_HOST_DEFINES: extra -D flags to check a tuning variant of the device library on the CPU
    extra = ["-D" + d for d in os.environ.get("CPZ_HOST_DEFINES", "").split() + list(defines)]
    _run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-DCPZ_BOUNDS_CHECK", "-DCPZ_COUNT_OPS"] + extra +
         ["-I", CSRC] + srcs + ["-o", tmp])
    os.replace(tmp, out)
    return out


def build_devprobe(force: bool = False, out: str = DEVPROBE, include: str = CSRC) -> str:
    """Device probes over the product headers (tests/native/devprobe.hip), compiled like the
    product's units.  `out` / `include` build the probes over another copy of the headers
    (a mutated one, or an earlier commit's) for tests/test_gpu_row_arith.py's CPZ_DEVPROBE."""
    src = os.path.join(ROOT, "tests", "native", "devprobe.hip")
    hdrs = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h")]
    if not force and not _newer(out, [src] + hdrs):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_partprobe(force: bool = False, out: str = PARTPROBE, include: str = CSRC) -> str:
    """Probes of the partitioned check's kernels (tests/native/partprobe.hip, which includes
    part.hip itself), compiled like the product's units.  `out` / `include` build them over
    another copy of csrc (a mutated one) for tests/test_gpu_part_probe.py's CPZ_PARTPROBE."""
    src = os.path.join(ROOT, "tests", "native", "partprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "part.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_partpairsprobe(force: bool = False, out: str = PARTPAIRSPROBE, include: str = CSRC) -> str:
    """Probes of the partitioned check's pair-mode kernels (tests/native/partpairsprobe.hip, which
    includes part.hip itself), compiled like the product's units.  `out` / `include` build them
    over another copy of csrc (a mutated one) for tests/test_gpu_part_pairs_probe.py's
    CPZ_PARTPAIRSPROBE."""
    src = os.path.join(ROOT, "tests", "native", "partpairsprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "part.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_partmanyprobe(force: bool = False, out: str = PARTMANYPROBE, include: str = CSRC) -> str:
    """Probes of the partitioned check's many-mode kernels (tests/native/partmanyprobe.hip, which
    includes part.hip itself), compiled like the product's units.  `out` / `include` build them
    over another copy of csrc (a mutated one) for tests/test_gpu_part_many_probe.py's
    CPZ_PARTMANYPROBE."""
    src = os.path.join(ROOT, "tests", "native", "partmanyprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "part.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_msmprobe(force: bool = False, out: str = MSMPROBE, include: str = CSRC) -> str:
    """Probes of the MSM's sort and reduction kernels (tests/native/msmprobe.hip, which includes
    rlc.hip itself), compiled like the product's units.  `out` / `include` build them over
    another copy of csrc (a mutated one) for tests/test_gpu_msm_probe.py's CPZ_MSMPROBE."""
    src = os.path.join(ROOT, "tests", "native", "msmprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "rlc.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_pairsumprobe(force: bool = False, out: str = PAIRSUMPROBE, include: str = CSRC) -> str:
    """Probe of the per-pair sum kernels of a mixed-pair batch over many pairs
    (tests/native/pairsumprobe.hip, which includes rlc.hip itself), compiled like the product's
    units.  `out` / `include` build it over another copy of csrc (a mutated one) for
    tests/test_gpu_pairsum_probe.py's CPZ_PAIRSUMPROBE."""
    src = os.path.join(ROOT, "tests", "native", "pairsumprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "rlc.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_prepprobe(force: bool = False, out: str = PREPPROBE, include: str = CSRC) -> str:
    """Probes of the batch check's prepare stage, the extras' kernels and the device scalar
    arithmetic (tests/native/prepprobe.hip, which includes rlc.hip itself), compiled like the
    product's units.  `out` / `include` build them over another copy of csrc (a mutated one) for
    tests/test_gpu_prep_probe.py's CPZ_PREPPROBE."""
    src = os.path.join(ROOT, "tests", "native", "prepprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "rlc.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


def build_microprobe(force: bool = False, out: str = MICROPROBE, include: str = CSRC) -> str:
    """Probes of the small per-pair generator tables of cpz_verify_each_pairs_many
    (tests/native/microprobe.hip, which includes kernels.hip itself), compiled like the product's
    units.  `out` / `include` build them over another copy of csrc (a mutated one) for
    tests/test_gpu_pair_micro_probe.py's CPZ_MICROPROBE."""
    src = os.path.join(ROOT, "tests", "native", "microprobe.hip")
    deps = [os.path.join(include, f) for f in os.listdir(include) if f.endswith(".h") or f == "kernels.hip"]
    if not force and not _newer(out, [src] + deps):
        return out
    tmp = out + ".tmp"
    _run([_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-I", include,
          "-I", os.path.join(ROOT, "include"), "-shared", src, "-o", tmp])
    os.replace(tmp, out)
    return out


CPP_TEST = os.path.join(ROOT, "tests", "cpp", "batch_verifier_test")


def build_cpp_test(force: bool = False) -> str:
    """C++ mirror of batch.rs's unit tests over include/cpz_batch.hpp (links libcpz.so)."""
    src = os.path.join(ROOT, "tests", "cpp", "batch_verifier_test.cpp")
    hdrs = [os.path.join(ROOT, "include", "cpz.h"), os.path.join(ROOT, "include", "cpz_batch.hpp")]
    # libcpz.so is linked dynamically: only the sources and headers make the binary stale (a rebuild
    # inside a GPU test run is what the in-tree build is there to avoid)
    if not force and not _newer(CPP_TEST, [src] + hdrs):
        return CPP_TEST
    cxx = shutil.which("g++") or "g++"
    _run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", CPP_TEST + ".tmp",
          "-L", LIBDIR, "-lcpz", "-Wl,-rpath,$ORIGIN/../../chaum-pedersen-zkp_amd/lib"])
    os.replace(CPP_TEST + ".tmp", CPP_TEST)
    return CPP_TEST


DROPIN_TEST = os.path.join(ROOT, "tests", "cpp", "dropin_test")


def build_dropin_test(force: bool = False) -> str:
    """The drop-in's call sequence through the C++ mirror (tests/test_gpu_dropin.py)."""
    src = os.path.join(ROOT, "tests", "cpp", "dropin_test.cpp")
    hdrs = [os.path.join(ROOT, "include", "cpz.h"), os.path.join(ROOT, "include", "cpz_batch.hpp")]
    if not force and not _newer(DROPIN_TEST, [src] + hdrs):  # libcpz.so: linked dynamically
        return DROPIN_TEST
    cxx = shutil.which("g++") or "g++"
    _run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", DROPIN_TEST + ".tmp",
          "-L", LIBDIR, "-lcpz", "-Wl,-rpath,$ORIGIN/../../chaum-pedersen-zkp_amd/lib"])
    os.replace(DROPIN_TEST + ".tmp", DROPIN_TEST)
    return DROPIN_TEST


MERGE_TEST = os.path.join(ROOT, "tests", "cpp", "merge_groups_test")


def build_merge_groups_test(force: bool = False) -> str:
    """The C++ mirror's merged dispatch against its per-group one (tests/test_gpu_pairs_cpp.py)."""
    src = os.path.join(ROOT, "tests", "cpp", "merge_groups_test.cpp")
    hdrs = [os.path.join(ROOT, "include", "cpz.h"), os.path.join(ROOT, "include", "cpz_batch.hpp")]
    if not force and not _newer(MERGE_TEST, [src] + hdrs):  # libcpz.so: linked dynamically
        return MERGE_TEST
    cxx = shutil.which("g++") or "g++"
    _run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", MERGE_TEST + ".tmp",
          "-L", LIBDIR, "-lcpz", "-Wl,-rpath,$ORIGIN/../../chaum-pedersen-zkp_amd/lib"])
    os.replace(MERGE_TEST + ".tmp", MERGE_TEST)
    return MERGE_TEST


def build_oracle(force: bool = False) -> None:
    mk = os.path.join(ROOT, "oracle", "Makefile")
    if os.path.exists(mk):
        _run(["make", "-s", "-C", os.path.join(ROOT, "oracle")] + (["-B"] if force else []))


def build_all(force: bool = False, verbose: bool = False) -> None:
    build_hosttest(force)
    build_oracle(force)
    build_libcpz(force, verbose)
    build_devprobe(force)
    build_partprobe(force)
    build_partpairsprobe(force)
    build_partmanyprobe(force)
    build_msmprobe(force)
    build_pairsumprobe(force)
    build_prepprobe(force)
    build_microprobe(force)
    build_cpp_test(force)
    build_dropin_test(force)
    build_merge_groups_test(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
