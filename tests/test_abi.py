"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/mapdit.h declares (no compute calls here: there is no GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mapdit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mapdit_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    import mapdit_amd
    L = mapdit_amd._lib
    if not os.path.exists(L.LIB_PATH):
        L.build()
    syms = declared_symbols()
    assert len(syms) >= 30
    cdll = ctypes.CDLL(L.LIB_PATH)
    for s in syms:
        assert hasattr(cdll, s), f"{s} declared in mapdit.h but not exported by libmapdit_hip.so"
    assert sorted(L.EXPORTS) == syms, set(L.EXPORTS) ^ set(syms)
    assert cdll.mapdit_abi_version() == 5


def test_no_compiler_generated_packed_fp32_code():
    """tools/check_packed_fp32.py on the built library: packed fp32 VALU arithmetic (v_pk_fma / mul / add_f32, v_pk_mov_b32) appears
    only in the hand-written SiLU + derivative GEMM epilogue.  Compiler-packed fp32 code produced wrong lane sums while a second
    process shared the GPU: the build flags that keep it out are a checked property, not a convention."""
    import subprocess
    import sys
    import mapdit_amd
    L = mapdit_amd._lib
    if not os.path.exists(L.LIB_PATH):
        L.build()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_packed_fp32.py"), L.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import mapdit_amd
    L = mapdit_amd._lib
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(L, "_handle", None)
    with pytest.raises(L.MapditError):
        L.lib()


def test_workspace_query_and_config_errors():
    import mapdit_amd
    L = mapdit_amd._lib
    lib = L.lib()
    cfg = L.Config(depth=12, hidden=768, patch=2, input_size=32, in_channels=4, num_heads=12, mlp_hidden=3072,
                   table_rows=1001, max_batch=32)
    train = lib.engine_workspace_bytes(ctypes.byref(cfg), 1)
    infer = lib.engine_workspace_bytes(ctypes.byref(cfg), 0)
    assert train > infer > 0
    assert train < 16 << 30
    xl = L.Config(depth=28, hidden=1152, patch=2, input_size=32, in_channels=4, num_heads=16, mlp_hidden=4608,
                  table_rows=1001, max_batch=2)
    assert lib.engine_workspace_bytes(ctypes.byref(xl), 0) > 0             # head_dim 72: generic attention path
    bad = L.Config(depth=2, hidden=200, patch=2, input_size=32, in_channels=4, num_heads=2, mlp_hidden=800,
                   table_rows=11, max_batch=2)
    assert lib.engine_workspace_bytes(ctypes.byref(bad), 0) == 0           # refused, not mis-computed
    assert b"hidden" in lib.last_error()
    big = L.Config(depth=2, hidden=256, patch=2, input_size=64, in_channels=4, num_heads=4, mlp_hidden=1024,
                   table_rows=11, max_batch=2)
    assert lib.engine_workspace_bytes(ctypes.byref(big), 0) > 0             # 1,024 tokens, head_dim 64: tiled MFMA attention
    big.num_heads = 8                                                      # head_dim 32 would need the generic kernels (<= 256 tokens)
    assert lib.engine_workspace_bytes(ctypes.byref(big), 0) == 0 and b"tokens" in lib.last_error()
    big.num_heads, big.input_size = 4, 36                                  # 324 tokens: not a multiple of 256
    assert lib.engine_workspace_bytes(ctypes.byref(big), 0) == 0 and b"tokens" in lib.last_error()


def test_build_is_decided_by_source_digest_not_file_times(monkeypatch):
    """build() keeps a SHA-256 of the sources next to the library and skips make while it matches: a repo snapshot copied to the
    GPU box does not keep file times, and nothing there should recompile a library that is current."""
    import subprocess
    import mapdit_amd._lib as L
    path = L.build()                                   # brings the stamp up to date (a no-op make at most)
    stamp = path + ".src-sha256"
    assert os.path.exists(path) and open(stamp).read().strip() == L._source_digest()
    calls = []
    monkeypatch.setattr(subprocess, "check_call", lambda *a, **k: calls.append(a))
    assert L.build() == path and calls == []           # current: make is not even started
    open(stamp, "w").write("stale\n")
    L.build()
    assert len(calls) == 1 and open(stamp).read().strip() == L._source_digest()


def test_gemm_tile_edge_rule():
    """mapdit_gemm_tile_size_k (host logic, no GPU): the documented decisions of the dispatcher on the DiT-B/2 shapes."""
    import mapdit_amd
    lib = mapdit_amd._lib.lib()
    t = lib.gemm_tile_size_k
    assert t(65536, 3072, 768, 0) == 256 and t(65536, 768, 3072, 0) == 256        # 256 samples: whole rounds of the chip
    assert t(8192, 768, 3072, 0) == 128                                            # 96 tiles of 256^2: under half a round
    assert t(8192, 2304, 768, 0) == 128                                            # 288 tiles: 1.125 rounds
    assert t(8192, 3072, 768, 0) == 256 and t(16384, 2304, 768, 0) == 256          # 1.5 and 2.25 rounds stay
    assert t(16, 768, 768, 0) == 128 and t(65536, 16, 768, 0) == 128               # conditioning path, final linear
    assert t(768, 768, 65536, 1) == 128                                            # split-K, smallest output
    assert t(3072, 768, 65536, 1) == 256 and t(3072, 768, 8192, 1) == 128          # 146 vs 18 K-tiles per workgroup
    assert lib.gemm_tile_size_ex(3072, 768, 1) == 256 and lib.gemm_tile_size(8192, 768) == 128   # older entry points (K unknown)


# ---- the header-derived binding (map-dit_amd/_abi.py) -------------------------------------------------------------------------------

_ORACLE_PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include <utility>
#include "mapdit.h"
template <class T> void kind() {
    if constexpr (std::is_pointer<T>::value) std::printf(" p");
    else if constexpr (std::is_void<T>::value) std::printf(" v");
    else std::printf(" %c%d", std::is_floating_point<T>::value ? 'f' : std::is_signed<T>::value ? 'i' : 'u', (int)sizeof(T));
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
    static void print(const char* name) { std::printf("fn %s", name); kind<R>(); (kind<A>(), ...); std::printf("\n"); }
};
struct any { template <class T> operator T() const; };                       /* converts to every field type: counts aggregate members */
template <class T, class = void, class... A> struct fields { static const int n = (int)sizeof...(A) - 1; };
template <class T, class... A> struct fields<T, decltype(void(T{std::declval<A>()...})), A...> : fields<T, void, A..., any> {};
int main() {
"""


def _kind(t):
    if t is None:
        return "v"
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "p"
    if t in (ctypes.c_float, ctypes.c_double):
        return f"f{ctypes.sizeof(t)}"
    return ("i" if t(-1).value < 0 else "u") + str(ctypes.sizeof(t))


def test_binding_equals_the_compilers_reading_of_the_header(tmp_path):
    """The oracle is a C++ compiler, not _abi.py's parser: a generated host program prints, from decltype(&mapdit_x), the kind of
    every function's return and parameters (p pointer, v void, i4 / i8 / u4 / u8 / f4 / f8), for every struct its size, its number
    of members and each member's offset and size, and every constant's value.  decltype names no function in an evaluated
    context, so the program links without the library.  Each line must equal what _lib bound with ctypes."""
    import shutil
    import subprocess
    import mapdit_amd
    L = mapdit_amd._lib
    if not os.path.exists(L.LIB_PATH):
        L.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mapdit.h")).read(), flags=re.S)
    funcs = declared_symbols()
    structs = sorted(set(re.findall(r"\}\s*(mapdit_\w+)\s*;", header)))
    consts = sorted(set(re.findall(r"\bMAPDIT_[A-Z0-9_]+\b", header)) - {"MAPDIT_H"})
    bound = {cls.__name__: cls for cls in vars(L).values() if isinstance(cls, type) and issubclass(cls, ctypes.Structure)}
    assert len(funcs) >= 151 and sorted(bound) == structs and len(structs) >= 8
    assert len(consts) >= 74 and all(type(getattr(L, c[len("MAPDIT_"):], None)) is int for c in consts)

    cdll = L.lib()._cdll
    body, expect = [], []
    for f in funcs:
        fn = getattr(cdll, f)
        body.append(f'sig<decltype(&{f})>::print("{f}");')
        expect.append(" ".join(["fn", f, _kind(fn.restype)] + [_kind(t) for t in fn.argtypes]))
    for s in structs:
        body.append(f'std::printf("struct {s} %zu %d\\n", sizeof({s}), fields<{s}>::n);')
        expect.append(f"struct {s} {ctypes.sizeof(bound[s])} {len(bound[s]._fields_)}")
        for name, t in bound[s]._fields_:
            body.append(f'std::printf("field {s}.{name} %zu %zu\\n", offsetof({s}, {name}), sizeof((({s}*)0)->{name}));')
            expect.append(f"field {s}.{name} {getattr(bound[s], name).offset} {ctypes.sizeof(t)}")
    for c in consts:
        body.append(f'std::printf("const {c} %lld\\n", (long long){c});')
        expect.append(f"const {c} {getattr(L, c[len('MAPDIT_'):])}")

    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no C++ compiler (CXX, c++, g++, clang++, hipcc) to read mapdit.h with"
    src = tmp_path / "abi_oracle.cpp"
    src.write_text(_ORACLE_PRELUDE + "\n".join(body) + "\nreturn 0;\n}\n")
    subprocess.run([*cxx.split(), "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi_oracle")],
                   check=True, capture_output=True, text=True)
    got = subprocess.run([str(tmp_path / "abi_oracle")], check=True, capture_output=True, text=True).stdout.splitlines()
    wrong = [(g, e) for g, e in zip(got, expect) if g != e]
    print(f"{len(funcs)} functions, {len(structs)} structs, {len(consts)} constants: {len(got)} lines, {len(wrong)} mismatches")
    assert len(got) == len(expect) and not wrong, wrong[:10]
    # which int results are statuses is the one thing the header does not say: the raw ctypes function for values, a raising wrapper else
    lib = L.lib()
    raw = sorted(f for f in funcs if getattr(lib, f[len("mapdit_"):]) is getattr(cdll, f))
    assert raw == sorted(L.VALUE_RETURNING | {f for f in funcs if getattr(cdll, f).restype is not ctypes.c_int})


def _abi():
    import mapdit_amd._abi as A
    return A


@pytest.mark.parametrize("snippet, quoted", [
    ("int mapdit_f(unsigned n, void* stream);", "unsigned"),                                    # an unknown scalar type
    ("int mapdit_f(mapdit_later_t* p);", "mapdit_later_t"),                                     # ... also behind a pointer
    ("typedef struct { int a[4]; } mapdit_s_t;", "int a[4]"),                                   # an array member
    ("typedef struct { int a : 3; } mapdit_s_t;", "int a : 3"),                                 # a bit-field
    ("int mapdit_f(int (*cb)(int), void* stream);", "int mapdit_f(int (*cb)(int), void* stream);"),   # a function-pointer parameter
    ("int mapdit_f(const char* fmt, ...);", "..."),                                             # variadic
    ("MAPDIT_F16_TWIN(mapdit_f);", "MAPDIT_F16_TWIN(mapdit_f);"),                               # a prototype produced by a macro
    ("MAPDIT_API int mapdit_f(int n);", "MAPDIT_API int"),
    ("int mapdit_f(int n);\nstray\nint mapdit_g(int n);", "stray int"),                         # a stray identifier between declarations
    ("stray;", "stray;"),
    ("typedef struct { int a; float b;", "typedef struct { int a;"),                            # an unterminated struct
    ("typedef struct { int a; float b } mapdit_s_t;", "float b"),
    ("enum { MAPDIT_A = 1 << 3 };", "MAPDIT_A = 1 << 3"),
    ("#define MAPDIT_X (1 + 2)", "#define MAPDIT_X (1 + 2)"),
    ("#pragma once", "#pragma once"),
    ("int mapdit_f(int n);\nint mapdit_f(int n);", "mapdit_f"),
    ("int mapdit_f(int n); /* unterminated", "/* unterminated"),
    ("}", "'}'"),
])
def test_reader_refuses_what_it_does_not_understand(snippet, quoted):
    A = _abi()
    with pytest.raises(A.AbiError) as e:
        A.parse("int mapdit_before(void);\n" + snippet)
    assert quoted in str(e.value), str(e.value)


def test_reader_enums_fields_and_types():
    A = _abi()
    abi = A.parse("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define MAPDIT_SLOTS 80 /* a comment */
        enum { A = 5, B, C = 0x10, D };   // 5, 6, 16, 17
        enum { E, F = -2, G };
        typedef struct { const uint16_t* A; int lda; int M, N; float alpha, beta;
                         long s; } pair_t;
        typedef struct tag handle_t;
        const char* name(void);
        void drop(handle_t* h);
        size_t need(const pair_t* p, int train);
        int run(handle_t** out, float* const* tab, uint64_t seed, double x, int64_t* idx);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert abi.constants == dict(MAPDIT_SLOTS=80, A=5, B=6, C=16, D=17, E=0, F=-2, G=-1)
    assert abi.structs == {"pair_t": [("A", "uint16_t*"), ("lda", "int"), ("M", "int"), ("N", "int"), ("alpha", "float"), ("beta", "float"),
                                      ("s", "long")]}
    assert abi.functions == {"name": ("char*", []), "drop": ("void", [("handle_t*", "h")]),
                             "need": ("size_t", [("pair_t*", "p"), ("int", "train")]),
                             "run": ("int", [("handle_t**", "out"), ("float**", "tab"), ("uint64_t", "seed"), ("double", "x"), ("int64_t*", "idx")])}
    assert [A.restype(r) for r in ("char*", "void", "size_t", "int")] == [ctypes.c_char_p, None, ctypes.c_size_t, ctypes.c_int]
    assert [A.ctype(t) for t in ("char*", "float**", "uint32_t", "long")] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_long]
    pair = A.structure("pair_t", abi.structs["pair_t"])
    assert pair(lda=3, alpha=0.5).lda == 3 and pair.s.offset == 32 and ctypes.sizeof(pair) == 40


def test_value_returning_must_be_declared_int():
    """Which int results are values is the one fact kept beside the header: a name in that set that the header declares with another
    return type (or not at all) stops the import."""
    import mapdit_amd
    L, A = mapdit_amd._lib, _abi()
    ok = "".join(f"int {n}(void);\n" for n in sorted(L.VALUE_RETURNING)) + "int mapdit_run(void* stream);\nvoid mapdit_drop(void* h);\n"
    assert L._status_returning(A.parse(ok)) == {"mapdit_run"}
    for bad in (ok.replace("int mapdit_gemm_dma_fast(", "long mapdit_gemm_dma_fast("), ok.replace("int mapdit_abi_version(void);\n", "")):
        with pytest.raises(A.AbiError):
            L._status_returning(A.parse(bad))


def test_importing_the_reader_loads_nothing():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import importlib.util as u, os; "
            "s = u.spec_from_file_location('_abi', os.path.join(%r, 'map-dit_amd', '_abi.py')); m = u.module_from_spec(s); s.loader.exec_module(m); "
            "assert 'torch' not in sys.modules and 'mapdit_amd' not in sys.modules; "
            "print(len(m.parse(open(os.path.join(%r, 'include', 'mapdit.h')).read()).functions))" % (ROOT, ROOT, ROOT))
    assert int(subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout) >= 151


def test_param_table_follows_the_header_slots():
    """DiT._param_table fills the engine's pointer table by slot name; the list it gives is the header's order."""
    import mapdit_amd
    from mapdit_amd.src.dit import DiT
    L = mapdit_amd._lib
    m = DiT(depth=2, hidden_size=64, patch_size=2, input_size=8, in_channels=4, num_heads=1, num_classes=10)
    f, t = m.final_layer, m.t_embedder
    want = [m.x_embedder.weight, t.mlp.net[0].weight, t.mlp.net[2].weight, m.y_embedder.embedding.weight, f.linear.weight,
            f.modulation[1].weight, f.mean_scale.linear.weight, f.mean_scale.reference, f.sigma_scale.linear.weight, f.sigma_scale.reference,
            f.gain_mod, t.embedding.scale, t.embedding.shift, m.pos_embed]
    for b in m.blocks:
        want += [b.attn.qkv_proj.weight, b.attn.out_proj.weight, b.mlp.net[0].weight, b.mlp.net[2].weight, b.modulation[1].weight,
                 b.gain_msa, b.gain_mlp]
    got = m._param_table()
    assert len(got) == len(want) == L.NUM_GLOBAL + 2 * L.NUM_BLOCK and all(a is b for a, b in zip(got, want))
