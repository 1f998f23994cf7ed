"""raytrace_amd._lib's signature tables against include/rt_abi.h, without a GPU and without loading a library: the `rt_` table names
exactly the functions the header declares, each with as many argtypes as the declaration has parameters; every entry of both tables
states its restype, and the host table names every `rth_` function the package calls."""
import ctypes as C
import os
import re

from raytrace_amd import _lib
from tests.conftest import ROOT


def _declarations():
    """{name: (return type, [parameter, ...])} of the header's function declarations, comments stripped."""
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z_0-9 ]*?[ \*]+)\s*\b(rt_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        assert name not in out, name
        out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


def test_the_rt_table_is_the_header():
    decl = _declarations()
    assert len(decl) >= 77
    assert sorted(_lib.AMD_FUNCTIONS) == sorted(decl)
    assert _lib.ABI_SYMBOLS == tuple(_lib.AMD_FUNCTIONS)
    for name, (ret, params) in sorted(decl.items()):
        restype, argtypes = _lib.AMD_FUNCTIONS[name]
        assert len(argtypes) == len(params), "%s: %d argtypes for (%s)" % (name, len(argtypes), ", ".join(params))
        assert (restype is None) == (ret == "void"), name
        if ret in ("int", "uint32_t", "uint64_t", "size_t"):
            assert restype is {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t}[ret], name
        elif ret != "void":
            assert "*" in ret and restype in (C.c_void_p, C.c_char_p), name
        for i, (p, a) in enumerate(zip(params, argtypes)):      # a pointer or array parameter is a pointer argtype, a value a value
            by_address = "*" in p or "[" in p
            is_pointer = a in (C.c_void_p, C.c_char_p) or isinstance(a, type(C.POINTER(C.c_int)))
            assert by_address == is_pointer, "%s: parameter %d (%s) against %r" % (name, i, p, a)
    assert _lib.AMD_FUNCTIONS["rt_abi_version"] == (C.c_uint32, [])


def test_every_entry_states_its_restype_and_argtypes():
    for table in (_lib.AMD_FUNCTIONS, _lib.HOST_FUNCTIONS):
        for name, entry in table.items():
            assert isinstance(entry, tuple) and len(entry) == 2 and isinstance(entry[1], list), name
            restype, argtypes = entry
            assert restype is None or issubclass(restype, C._SimpleCData), name
            assert all(isinstance(a, type) for a in argtypes), name


def test_the_host_table_covers_every_rth_call_of_the_package():
    called = set()
    pkg = os.path.join(ROOT, "raytrace_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py") and f != "_lib.py":
            called |= set(re.findall(r"\b(rth_[a-z_0-9]+)\s*\(", open(os.path.join(pkg, f)).read()))
    assert len(called) >= 50
    assert called <= set(_lib.HOST_FUNCTIONS), sorted(called - set(_lib.HOST_FUNCTIONS))
    defined = set(re.findall(r"^[A-Za-z_][\w \*]*?\b(rth_[a-z_0-9]+)\s*\(", open(os.path.join(pkg, "host", "host_capi.cpp")).read(), flags=re.M))
    assert set(_lib.HOST_FUNCTIONS) <= defined, sorted(set(_lib.HOST_FUNCTIONS) - defined)
