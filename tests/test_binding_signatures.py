"""The binding's signature table (ulc_amd.SIGNATURES) held against the prototypes of include/ulc_amd.h: the same functions, and
for each the same arity, the same class of every argument, a matching return type and, where the table types a pointer, the
header's element type.  No GPU and no library: the table is built at import."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import ulc_amd

HEADER = os.path.join(ROOT, "include", "ulc_amd.h")
# scalar classes: the header's type words -> the ctypes that may stand for them (c_int32 is c_int and c_int64 c_longlong on this ABI)
SCALARS = {"int": (C.c_int,), "int32_t": (C.c_int32,), "float": (C.c_float,), "long long": (C.c_longlong,), "size_t": (C.c_size_t,),
           "uint32_t": (C.c_uint32,), "uint64_t": (C.c_uint64,)}
ELEMENTS = {"float": C.c_float, "int32_t": C.c_int32, "uint8_t": C.c_uint8, "int64_t": C.c_int64, "double": C.c_double}
RETURNS = {"const char *": C.c_char_p, "size_t": C.c_size_t, "const void *": C.c_void_p, "void": None, "int": C.c_int}


def prototypes():
    """name -> (return type, [parameter text]) of every function the header declares."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s*\b((?:ULC|ulcx)_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(a.split()) for a in args.split(",")]
        if params == ["void"] or params == [""]:
            params = []
        assert name not in found, name
        found[name] = (" ".join(ret.replace("*", " * ").split()), params)
    return found


def scalar_class(param):
    words = re.sub(r"\bconst\b", " ", param).split()[:-1]              # (the last word is the parameter's name)
    return " ".join(words)


def is_pointer(param):
    return "*" in param or "[" in param


def is_ctypes_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or isinstance(t, type(C.POINTER(C.c_int)))


PROTOS = prototypes()


def test_the_header_and_the_table_name_the_same_functions():
    assert len(PROTOS) == 149
    assert set(PROTOS) == set(ulc_amd.EXPORTS)
    assert len(ulc_amd.EXPORTS) == len(set(ulc_amd.EXPORTS))
    assert set(ulc_amd.SIGNATURES) == set(ulc_amd.EXPORTS)
    for dev, twin in ulc_amd.PCM16_TWIN.items():
        assert dev in PROTOS and twin in PROTOS and "pcm16" in twin and "pcm16" not in dev, (dev, twin)
        assert ulc_amd.SIGNATURES[twin] == ulc_amd.SIGNATURES[dev], (dev, twin)
        assert len(PROTOS[twin][1]) == len(PROTOS[dev][1]), (dev, twin)
    assert sorted(ulc_amd.PCM16_TWIN.values()) == sorted(n for n in PROTOS if "pcm16" in n)


def test_every_entry_has_the_headers_arity_and_argument_classes():
    for name, (ret, params) in PROTOS.items():
        argtypes, _ = ulc_amd.SIGNATURES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for k, (t, param) in enumerate(zip(argtypes, params)):
            if is_pointer(param):
                assert is_ctypes_pointer(t), (name, k, param, t)
            else:
                assert scalar_class(param) in SCALARS, (name, k, param)
                assert t in SCALARS[scalar_class(param)], (name, k, param, t)


def test_every_entry_has_the_headers_return_type():
    for name, (ret, _) in PROTOS.items():
        assert ret in RETURNS, (name, ret)
        assert ulc_amd.SIGNATURES[name][1] is RETURNS[ret], (name, ret, ulc_amd.SIGNATURES[name][1])


def test_a_typed_pointer_points_at_the_headers_element_type():
    typed = 0
    for name, (_, params) in PROTOS.items():
        for k, (t, param) in enumerate(zip(ulc_amd.SIGNATURES[name][0], params)):
            if not is_pointer(param) or t in (C.c_void_p, C.c_char_p):
                continue
            words = re.sub(r"\bconst\b|\*|\[\w*\]", " ", param).split()[:-1]
            if len(words) == 1 and words[0] in ELEMENTS:
                assert t._type_ is ELEMENTS[words[0]], (name, k, param, t)
                typed += 1
    assert typed >= 2 * sum(n.endswith("_host") for n in PROTOS), typed    # (every host form has two typed buffers or more)
