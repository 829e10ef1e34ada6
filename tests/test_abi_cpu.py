"""CPU-side checks of the C-ABI library: it loads without a GPU and exports every symbol that
include/tt.h declares; the Python binding table mirrors the header.  No compute calls here."""
import ctypes
import re

import pytest

from conftest import ROOT


def _declared(header="tt.h"):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_functions():
    names = _declared()
    assert "tt_score_topk_f32" in names and "tt_last_error" in names and len(names) >= 6


def test_library_exports_every_declared_symbol(libtt):
    for header in sorted(p.name for p in (ROOT / "include").glob("*.h")):
        for name in _declared(header):
            assert hasattr(libtt, name), f"libtt.so does not export {name} ({header})"


def test_debug_exports_are_not_part_of_the_product_surface():
    """include/tt_debug.h is test infrastructure: the package binds none of it."""
    from twotowermlretrieval_amd import _lib
    dbg = _declared("tt_debug.h")
    assert dbg and all(n.startswith("tt_debug_") for n in dbg)
    assert not set(dbg) & set(_lib.SIGNATURES)
    for f in (ROOT / "twotowermlretrieval_amd").glob("*.py"):
        assert "tt_debug_" not in f.read_text(), f


def test_binding_table_matches_header():
    from twotowermlretrieval_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


_PTR = ("pointer", ctypes.sizeof(ctypes.c_void_p), None)
# what a by-value C type of the header is to the calling convention: (kind, bytes, signed -- None where there is no sign)
_C_VALUE_TYPES = {"int": ("int", 4, True), "int32_t": ("int", 4, True), "uint32_t": ("int", 4, False),
                  "int64_t": ("int", 8, True), "uint64_t": ("int", 8, False), "size_t": ("int", ctypes.sizeof(ctypes.c_size_t), False),
                  "float": ("float", 4, None), "char": ("char", 1, None), "tt_stream_t": _PTR}


def _c_shape(decl, named):
    """(kind, bytes, signed) of one C parameter declaration (`named`: it ends in the parameter's name) or return type."""
    if "*" in decl:
        return _PTR
    words = [w for w in decl.split() if w != "const"]
    if named:
        assert len(words) == 2, f"cannot read the parameter {decl!r}"
        words = words[:1]
    assert len(words) == 1 and words[0] in _C_VALUE_TYPES, f"a type this test does not know: {decl!r}"
    return _C_VALUE_TYPES[words[0]]


def _ctypes_shape(t):
    """The same triple of a ctypes type of the binding table."""
    code = t._type_
    if code in "Pz":                                             # c_void_p, c_char_p
        return _PTR
    if code == "f":
        return ("float", ctypes.sizeof(t), None)
    if code == "c":
        return ("char", ctypes.sizeof(t), None)
    assert code in "bhilqBHILQ", f"a ctypes type this test does not know: {t}"
    return ("int", ctypes.sizeof(t), code.islower())


def _prototypes(header="tt.h"):
    """name -> (return shape or None for void, [argument shapes]) of every function the header declares."""
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(tt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, args = " ".join(ret.split()), [" ".join(a.split()) for a in args.split(",")]
        assert name not in out, f"{name} is declared twice"
        out[name] = (None if ret == "void" else _c_shape(ret, False), [] if args == ["void"] else [_c_shape(a, True) for a in args])
    return out


def test_binding_table_matches_header_prototypes():
    """Every argument of every prototype: the table's ctypes type has the kind (pointer, integer, float, char), the size
    and the signedness of the header's C type, and so has the return type.  An `int` in the table where the header says
    int64_t truncates a row count or an offset only past 2^31, where no small test would see it."""
    from twotowermlretrieval_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == _declared() == sorted(_lib.SIGNATURES)
    for name, (c_res, c_args) in protos.items():
        res, args = _lib.SIGNATURES[name]
        assert (None if res is None else _ctypes_shape(res)) == c_res, f"{name}: return type"
        assert len(args) == len(c_args), f"{name}: {len(args)} arguments bound, {len(c_args)} declared"
        for n, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_shape(a) == c, f"{name}: argument {n} is bound as {a.__name__}, the header says {c}"


def test_prototype_reader_tells_the_types_apart():
    """The reader itself: the shapes it gives to the declarations a wrong table entry would be confused with."""
    assert _c_shape("int64_t N", True) != _c_shape("int N", True) and _c_shape("size_t n", True) != _c_shape("int64_t n", True)
    assert _c_shape("uint64_t seed", True) == _c_shape("size_t n", True) == _ctypes_shape(ctypes.c_uint64)
    assert _c_shape("const float *const *w", True) == _c_shape("tt_stream_t stream", True) == _ctypes_shape(ctypes.c_void_p)
    assert _ctypes_shape(ctypes.c_int) == _c_shape("int", False) != _ctypes_shape(ctypes.c_int64) == _c_shape("int64_t", False)
    assert _c_shape("float margin", True) == _ctypes_shape(ctypes.c_float) and _c_shape("char sep", True) == _ctypes_shape(ctypes.c_char)
    assert _c_shape("const char *", False) == _ctypes_shape(ctypes.c_char_p)


def test_version_and_error_strings(libtt):
    assert b"gfx950" in libtt.tt_version()
    assert isinstance(libtt.tt_last_error(), bytes)


def test_workspace_query_needs_no_gpu(libtt):
    n = libtt.tt_score_topk_workspace_bytes(32, 1_000_000, 256, 10)
    assert n > 0 and n % 8 == 0
    assert libtt.tt_score_topk_workspace_bytes(0, 10, 256, 10) == 0


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    rc = libtt.tt_score_topk_f32(None, 4, 100, None, 10, 5, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED and b"d=100" in libtt.tt_last_error()
    rc = libtt.tt_score_topk_f32(None, 4, 256, None, 10, 65, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0, None)
    assert rc == _lib.TT_ERR_UNSUPPORTED
    rc = libtt.tt_topk_merge(None, None, -1, 0, 5, None, None, None)
    assert rc == _lib.TT_ERR_BAD_SHAPE


def test_product_refuses_cpu_tensors():
    import torch
    import twotowermlretrieval_amd as tt
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.score_topk(torch.zeros(2, 256), torch.zeros(10, 256), 5)


def test_product_never_imports_oracle():
    pkg = ROOT / "twotowermlretrieval_amd"
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")):
        src = f.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
        assert "tt_oracle" not in src or f.suffix != ".py", f


def test_header_is_plain_c_and_links_against_the_library(tmp_path):
    """include/tt.h is the contract: it must compile as C99 (no C++ or torch types) and a C program that calls
    through it must link against libtt.so and run (host-only entry points: version string, error string,
    workspace queries, the tokenizer)."""
    import shutil
    import subprocess
    from twotowermlretrieval_amd import build as b
    lib = b.build()
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "abi.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "tt.h"
int main(void)
{
    const char *words = "theofw5";
    const int64_t off[4] = {0, 3, 5, 7}, ids[3] = {0, 3, 5};
    void *h = 0;
    if (tt_tok_create(words, off, ids, 3, 9, &h) != 0) return 2;
    const char *text = "The w5, of zzz";
    const int64_t toff[2] = {0, (int64_t)strlen(text)};
    int64_t ragged[32]; int32_t len = 0, status = 0;
    if (tt_tok_encode(h, text, toff, 1, ragged, &len, &status, 1) != 0) return 3;
    tt_tok_destroy(h);
    /* "The w5, of zzz" -> the w5 , of zzz -> 0 5 <unk=9> 3 9 */
    if (status != 0 || len != 5 || ragged[0] != 0 || ragged[1] != 5 || ragged[2] != 9 || ragged[3] != 3 || ragged[4] != 9) return 4;
    if (tt_score_topk_workspace_bytes(1024, 10000000, 256, 10) == 0) return 5;
    if (tt_score_topk_f32(0, 1, 7, 0, 1, 10, 0, 0, 0, 0, 0, 0) == 0) return 6;      /* d = 7 is refused ... */
    if (strstr(tt_last_error(), "d=7") == 0) return 7;                               /* ... with a message */
    printf("%s\n", tt_version());
    return 0;
}
""")
    exe = tmp_path / "abi"
    inc = b.PKG.parent / "include"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{inc}", str(src), "-o", str(exe), str(lib),
                        f"-Wl,-rpath,{lib.parent}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip()
