"""The Rust side of the boundary (rust/): no Rust toolchain exists in this image, so the
crates are checked mechanically -- every function and constant of include/cpz.h appears in
the -sys crate's extern block with the same parameter list (C types mapped to their Rust
FFI equivalents), the build script compiles exactly the HIP units the library is made of,
and the reference-side patch contains no `unsafe` (the reference crate is
#![forbid(unsafe_code)], src/lib.rs:64)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYS = os.path.join(ROOT, "rust", "chaum-pedersen-gpu-sys")


def _strip_c_comments(s):
    return re.sub(r"/\*.*?\*/", "", s, flags=re.S)


def _c_decls():
    src = _strip_c_comments(open(os.path.join(ROOT, "include", "cpz.h")).read())
    out = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(cpz_\w+)\s*\((.*?)\);", src, flags=re.S | re.M):
        args = " ".join(args.split())
        out[name] = (" ".join(ret.split()), [] if args == "void" else [a.strip() for a in args.split(",")])
    return out


def _c_defines():
    src = open(os.path.join(ROOT, "include", "cpz.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (CPZ_\w+) \(?(-?\d+)\)?", src)}


def _c_param_to_rust(p):
    """(name, rust type) of one C parameter."""
    m = re.match(r"^(const\s+)?(\w+)\s*(\*\s*const\s*\*|\*\*|\*)?\s*(\w+)(\[[^\]]*\])?$", p)
    assert m, p
    const, base, stars, name, arr = m.groups()
    stars = (stars or "").replace(" ", "")
    prim = {"uint8_t": "u8", "uint32_t": "u32", "uint64_t": "u64", "size_t": "usize", "int": "c_int",
            "double": "f64", "void": "c_void", "cpz_ctx": "cpz_ctx"}[base]
    if stars == "*const*":
        return name, "*const *mut " + prim
    if stars == "**":
        return name, "*mut *mut " + prim
    if stars == "*" or arr:
        return name, ("*const " if const else "*mut ") + prim
    return name, prim


def _c_ret_to_rust(r):
    return {"int": "c_int", "void": None, "const char *": "*const c_char"}[r]


def _rust_decls():
    src = open(os.path.join(SYS, "src", "lib.rs")).read()
    block = src[src.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (cpz_\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split())
        params = [] if not args else [tuple(x.strip() for x in a.split(":", 1)) for a in args.split(",") if a.strip()]
        out[name] = (" ".join(ret.split()) or None, params)
    consts = {k: int(v) for k, v in re.findall(r"pub const (CPZ_\w+): \w+ = (-?\d+);", src)}
    return out, consts


def test_extern_block_matches_header():
    c = _c_decls()
    r, _ = _rust_decls()
    assert set(c) == set(r), (sorted(set(c) - set(r)), sorted(set(r) - set(c)))
    for name, (ret, params) in c.items():
        rret, rparams = r[name]
        assert rret == _c_ret_to_rust(ret), (name, ret, rret)
        want = [_c_param_to_rust(p) for p in params]
        assert [tuple(p) for p in rparams] == want, (name, rparams, want)


def test_constants_match_header():
    _, consts = _rust_decls()
    defs = _c_defines()
    assert set(defs) == set(consts), (sorted(set(defs) - set(consts)), sorted(set(consts) - set(defs)))
    for k, v in defs.items():
        assert consts[k] == v, k


def test_build_script_compiles_the_library_units():
    import build_native  # the in-tree recipe: the same translation units
    b = open(os.path.join(SYS, "build.rs")).read()
    units = re.search(r"const UNITS: \[&str; \d+\] = \[(.*?)\];", b).group(1)
    units = [u.strip().strip('"') for u in units.split(",")]
    csrc = os.path.join(ROOT, "chaum-pedersen-zkp_amd", "csrc")
    assert sorted(units) == sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert "gfx950" in b and 'links = "cpz"' in open(os.path.join(SYS, "Cargo.toml")).read()
    assert "kernels.hip" in open(build_native.__file__).read()


def test_reference_patch_is_safe_code():
    for rel in ("rust/reference-patch/gpu.rs", "rust/reference-patch/dispatch.rs"):
        src = open(os.path.join(ROOT, rel)).read()
        code = "\n".join(l.split("//")[0] for l in src.splitlines())
        assert "unsafe" not in code, rel
    wrap = open(os.path.join(ROOT, "rust", "chaum-pedersen-gpu", "src", "lib.rs")).read()
    # every unsafe block in the safe wrapper carries a SAFETY note
    lines = wrap.splitlines()
    for i, l in enumerate(lines):
        if "unsafe {" in l and "impl" not in l:
            ctx = "\n".join(lines[max(0, i - 3):i + 1])
            assert "SAFETY" in ctx, (i, l)


VERIFY_SIG = "pub fn verify<R: CryptoRngCore>(&self, rng: &mut R) -> Result<Vec<Result<()>>>"


def _code(rel):
    src = open(os.path.join(ROOT, rel)).read()
    return "\n".join(l.split("//")[0] for l in src.splitlines())


def test_patch_serves_verify_with_the_reference_signature():
    """The drop-in is `verify` itself (batch.rs:171), not a new method: callers need no edit.
    Its signature is the reference's (VERIFY_SIG, pinned here), and it dispatches to the GPU
    under the feature and to the renamed CPU body otherwise."""
    d = _code("rust/reference-patch/dispatch.rs")
    assert " ".join(d.split()).count(VERIFY_SIG) == 1
    assert '#[cfg(feature = "gpu")]' in d and "super::gpu::verify(self, rng)" in d
    assert '#[cfg(not(feature = "gpu"))]' in d and "self.verify_cpu(rng)" in d
    g = _code("rust/reference-patch/gpu.rs")
    assert "verify_gpu" not in g and "verify_gpu" not in d


def test_patch_draws_the_seed_from_rng_and_uses_the_batch_check():
    g = _code("rust/reference-patch/gpu.rs")
    # rng drawn as the reference draws it: one 64-byte random_scalar per entry for n >= 2
    # (batch.rs:239-240), the first 32 bytes keying the weights
    assert "let mut draw = [0u8; 64];" in g and "for i in 0..entries.len() {" in g
    assert "rng.fill_bytes(&mut draw);" in g and "seed.copy_from_slice(&draw[..32]);" in g
    assert "gpu.verify_each_with(EQUATIONS_ONLY," in g   # Proof::new entries: equations only, per call
    assert ".verify_batch_with(EQUATIONS_ONLY," in g
    assert "set_commitment_checks" not in g              # never the shared context mode
    assert "if rows.len() < RLC_MIN_GROUP {" in g
    assert "if entries.len() == 1 {" in g and "OsRng.fill_bytes(&mut seed)" in g   # n == 1: rng untouched
    assert "first_index += rows.len() as u64;" in g      # consecutive weight indices, every group


def test_patch_pools_contexts_over_every_gpu():
    """gpu.rs keeps CONTEXTS_PER_DEVICE (>= 2) contexts on every visible GPU and checks one
    out per verify call, instead of one static context on GPU 0; its RLC threshold is the
    C++ mirror's and the Python mirror's (the call sequence tests/test_gpu_dropin.py runs)."""
    g = _code("rust/reference-patch/gpu.rs")
    m = re.search(r"const CONTEXTS_PER_DEVICE: usize = (\d+);", g)
    assert m and int(m.group(1)) >= 2
    assert "for d in 0..devices" in g and "device_count()" in g
    assert "pool()?.checkout()" in g and "try_lock()" in g
    assert "Gpu::new(0)" not in g
    rust_min = int(re.search(r"const RLC_MIN_GROUP: usize = (\d+);", g).group(1))
    hpp = open(os.path.join(ROOT, "include", "cpz_batch.hpp")).read()
    assert int(re.search(r"constexpr std::size_t RLC_MIN_GROUP = (\d+);", hpp).group(1)) == rust_min
    import chaum_pedersen as cp
    assert cp.RLC_MIN_GROUP == rust_min
    # the safe crate exposes the per-call flag the patch uses
    wrap = open(os.path.join(ROOT, "rust", "chaum-pedersen-gpu", "src", "lib.rs")).read()
    assert "pub const EQUATIONS_ONLY: CallFlags = sys::CPZ_CALL_EQUATIONS_ONLY;" in wrap


def test_patch_compresses_generators_once_per_group():
    """g and h are compressed in compress_generators only, which runs when a new Parameters
    group is created -- never inside the per-entry row building."""
    g = _code("rust/reference-patch/gpu.rs")
    lines = g.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("fn compress_generators"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("}"))
    for i, l in enumerate(lines):
        if "generator_g()" in l or "generator_h()" in l:
            inside = start <= i <= end
            grouping = "e.params.generator_g(), e.params.generator_h()" in l   # Element refs, no compression
            assert inside or grouping, (i, l)
            assert "element_to_bytes" not in l or inside, (i, l)
    calls = [l for l in lines if "compress_generators(" in l and not l.startswith("fn ")]
    assert len(calls) == 1 and "None =>" in calls[0]
    rows = lines[next(i for i, l in enumerate(lines) if l.startswith("fn entry_rows")):]
    rows = rows[:next(i for i, l in enumerate(rows) if l.startswith("}"))]
    assert not any("generator" in l for l in rows)
