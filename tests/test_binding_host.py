"""CPU test of the binding's signature tables: every prototype of include/if_fir.h and include/if_fir_debug.h has an entry in
if_fir.ABI / if_fir.DEV_ABI of the same arity, the same scalar types and the same return type.  No library is loaded."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32,
           "double": ctypes.c_double}
PROTOTYPE = re.compile(r"([\w ]+?[\s*]+)\b(if_(?:fir|bpf)_\w+)\s*\(([^()]*)\)\s*;")


def prototypes(header):
    """{name: (return type, [parameter types])} of a header, the types as C text without the parameter names"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for ret, name, params in PROTOTYPE.findall(text):
        params = [" ".join(p.split()) for p in params.split(",")]
        params = [] if params == ["void"] else [re.sub(r"\w+$", "", p).strip() for p in params]
        assert name not in found, name
        found[name] = (" ".join(ret.split()), params)
    return found


def is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


@pytest.mark.parametrize("header, table, count", [("if_fir.h", "ABI", 214), ("if_fir_debug.h", "DEV_ABI", 33)])
def test_every_prototype_has_its_signature(fir, header, table, count):
    declared = prototypes(header)
    table = getattr(fir, table)
    assert len(declared) == count
    assert set(declared) == set(table), set(declared) ^ set(table)
    for name, (ret, params) in declared.items():
        restype, argtypes = table[name]
        assert len(argtypes) == len(params), name
        for c, t in zip(params, argtypes):
            if c.endswith("*"):
                assert is_pointer(t), (name, c, t)
            else:
                assert t is SCALARS[c], (name, c, t)
        if ret == "void":
            assert restype is None, name
        elif ret == "const char *":
            assert restype is ctypes.c_char_p, name
        elif ret.endswith("*"):
            assert restype is ctypes.c_void_p, name
        else:
            assert restype is SCALARS[ret], (name, ret, restype)


def test_export_lists_are_the_tables(fir):
    assert list(fir.EXPORTS) == list(fir.ABI) and list(fir.DEV_EXPORTS) == list(fir.DEV_ABI)
    assert not set(fir.ABI) & set(fir.DEV_ABI)
