"""CPU, no built library: the ctypes binding that de_i2i_gan_amd._lib derives from include/dei2i_hip.h, checked by a C++ compiler.
One generated translation unit includes the header and static_asserts, for every entry of SIGNATURES, the arity and the ABI class
of the return value and of every parameter; for every derived Structure its sizeof, every field's offsetof and ABI class; for every
constant its DEI2I_* macro.  The parser cannot pass by agreeing with itself: g++ reads the same header.  Then the refusals: what the
parser does not know raises and names the token, it never becomes a pointer or an int."""
import ctypes
import importlib.util
import shutil
import subprocess
from pathlib import Path

import pytest

from de_i2i_gan_amd import _lib

REPO = Path(__file__).resolve().parents[1]

TRAITS = r"""
#include <cstddef>
#include <type_traits>
#include "dei2i_hip.h"
enum Cls { VOID, PTR, I32, I64, U64, F32, F64, OTHER };
template <class T> constexpr Cls cls() {
  if constexpr (std::is_void_v<T>) return VOID;
  else if constexpr (std::is_pointer_v<T>) return PTR;
  else if constexpr (std::is_same_v<T, float>) return F32;
  else if constexpr (std::is_same_v<T, double>) return F64;
  else if constexpr (std::is_same_v<T, bool> || !std::is_integral_v<T>) return OTHER;
  else if constexpr (std::is_signed_v<T> && sizeof(T) == 4) return I32;
  else if constexpr (std::is_signed_v<T> && sizeof(T) == 8) return I64;
  else if constexpr (std::is_unsigned_v<T> && sizeof(T) == 8) return U64;
  else return OTHER;
}
template <class F> struct fn;
template <class R, class... A> struct fn<R (*)(A...)> {
  static constexpr int arity = sizeof...(A);
  static constexpr Cls ret = cls<R>();
  static constexpr Cls arg[sizeof...(A) + 1] = {cls<A>()..., OTHER};
};
"""


def abi_class(t):
    """the ABI class (an enumerator of Cls above) a ctypes type stands for"""
    if t is None:
        return "VOID"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "PTR"
    if t in (ctypes.c_float, ctypes.c_double):
        return "F32" if t is ctypes.c_float else "F64"
    assert issubclass(t, ctypes._SimpleCData) and isinstance(t(0).value, int), t
    return {(True, 4): "I32", (True, 8): "I64", (False, 8): "U64"}[(t(-1).value < 0, ctypes.sizeof(t))]


def translation_unit(constants, structs, signatures):
    out = [TRAITS]
    for name, value in constants.items():
        out.append(f'static_assert(DEI2I_{name} == {value}, "DEI2I_{name}");')
    for name, st in structs.items():
        out.append(f'static_assert(sizeof({name}) == {ctypes.sizeof(st)}, "sizeof {name}");')
        for field, ctype in st._fields_:
            out.append(f'static_assert(offsetof({name}, {field}) == {getattr(st, field).offset}, "offsetof {name}.{field}");')
            out.append(f'static_assert(cls<decltype({name}::{field})>() == {abi_class(ctype)}, "class of {name}.{field}");')
    for name, (res, args) in signatures.items():
        f = f"fn<decltype(&{name})>"
        out.append(f'static_assert({f}::arity == {len(args)}, "{name} arity");')
        out.append(f'static_assert({f}::ret == {abi_class(res)}, "{name} return");')
        out += [f'static_assert({f}::arg[{i}] == {abi_class(a)}, "{name} arg {i}");' for i, a in enumerate(args)]
    return "\n".join(out) + "\n"


def compile_unit(source, tmp_path):
    assert shutil.which("g++"), "g++ is missing: the build needs it for tests/hostcheck, so this is a failure, not a skip"
    path = tmp_path / "abi_check.cpp"
    path.write_text(source)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", str(REPO / "include"), str(path)], capture_output=True, text=True)


def test_derived_binding_matches_the_compilers_reading_of_the_header(tmp_path):
    assert len(_lib.SIGNATURES) >= 118 and len(_lib.STRUCTS) >= 6 and len(_lib.CONSTANTS) >= 21
    run = compile_unit(translation_unit(_lib.CONSTANTS, _lib.STRUCTS, _lib.SIGNATURES), tmp_path)
    assert run.returncode == 0, run.stderr[-4000:]


def test_module_attributes_are_the_parsed_ones():
    for name, value in _lib.CONSTANTS.items():
        assert getattr(_lib, name) == value, name
    assert (_lib.ERR_BAD_ARG, _lib.ERR_WORKSPACE, _lib.EMBED_MAX_LABEL_NC, _lib.DIGEST_MAX_ROWS) == (-2, -3, 16, 65535)
    named = dict(ConvDesc="dei2i_conv", ProDesc="dei2i_pro", EpiNormDesc="dei2i_epi_norm", LabelMod="dei2i_label_mod",
                 AdamRec="dei2i_adam_rec", DiffAugRec="dei2i_diffaug_rec")
    for attr, c_name in named.items():
        assert getattr(_lib, attr) is _lib.STRUCTS[c_name], attr
    assert set(named.values()) == set(_lib.STRUCTS)
    assert _lib.ADAM_REC_WORDS * 8 == ctypes.sizeof(_lib.AdamRec)
    res, args = _lib.SIGNATURES["dei2i_conv2d_fwd"]                      # descriptors are typed, strings are strings, the rest is void*
    assert res is ctypes.c_int and args[0]._type_ is _lib.ConvDesc and args[1] is ctypes.c_void_p and args[7] is ctypes.c_size_t
    assert _lib.SIGNATURES["dei2i_set_option"] == (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int])
    assert _lib.SIGNATURES["dei2i_error_string"] == (ctypes.c_char_p, [ctypes.c_int])
    assert _lib.SIGNATURES["dei2i_launch_counts_reset"] == (None, [])


@pytest.mark.parametrize("snippet, names", [
    ("int dei2i_f(int n, unsigned short k);", ["dei2i_f", "'short'"]),                                   # an unknown type token
    ("int dei2i_a(int x)\nint dei2i_b(int y);", ["dei2i_a", "';'", "'int'"]),                            # a prototype without ;
    ("int dei2i_a(int x);\nint dei2i_b(int y)", ["';'", "at the end"]),
    ("typedef struct dei2i_s {\n  int a, b;\n  uint16_t c;\n} dei2i_s;", ["dei2i_s", "'uint16_t'"]),      # a field of an unknown type
    ("typedef struct dei2i_s {\n  int a, *b;\n} dei2i_s;", ["dei2i_s", "'*b'"]),
    ("int dei2i_f(int*);", ["dei2i_f", "no name"]),                                                      # would read `int` as the name
    ("int dei2i_f(unsigned char c);", ["dei2i_f", "'unsigned char'"]),                                   # a pointee only
    ("typedef struct dei2i_s { int a; } dei2i_s;\nint dei2i_f(dei2i_s by_value);", ["dei2i_f", "'dei2i_s'"]),
    ("#define DEI2I_LIMIT 1u << 4", ["DEI2I_LIMIT", "not an integer"]),
])
def test_parser_refuses_what_it_does_not_know(snippet, names):
    with pytest.raises(ValueError) as err:
        _lib.parse_header(snippet)
    for name in names:
        assert name in str(err.value), (name, str(err.value))


def test_missing_header_is_an_error_that_names_the_path(tmp_path):
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(_lib.__file__, pkg / "_lib.py")
    spec = importlib.util.spec_from_file_location("_lib_without_header", pkg / "_lib.py")
    with pytest.raises(RuntimeError, match="dei2i_hip.h") as err:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert str(tmp_path / "include" / "dei2i_hip.h") in str(err.value)
