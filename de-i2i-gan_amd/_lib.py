"""ctypes binding of libdei2i_hip.so, derived at import from its C ABI, include/dei2i_hip.h: every prototype -> SIGNATURES, every
struct -> a ctypes.Structure, every integer `#define DEI2I_<NAME>` -> <NAME>.  Fails loudly when the header or the library is missing."""
import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_longlong, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdei2i_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "dei2i_hip.h"))

# The header's whole type vocabulary; a token outside it raises (it never defaults to a pointer or an int).
_SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "int64_t": c_int64, "uint64_t": c_uint64,
            "long long": c_longlong, "dei2i_stream": c_void_p}
_POINTEES = {"void", "unsigned char"} | set(_SCALARS)            # what a plain pointer (-> c_void_p) may point at
_WORDS = {word for base in _POINTEES for word in base.split()}
# The descriptors a caller hands over one at a time with byref(): pointers to them are typed.  The other structs are rows of tables
# that are passed by address (most live in device memory), so pointers to them are c_void_p like every other pointer.
_BYREF_STRUCTS = {"dei2i_conv", "dei2i_pro", "dei2i_epi_norm"}


def _ctype(tokens, structs, where):
    """The ctypes type of a C type given as tokens: descriptor pointer -> POINTER(Structure), const char* -> c_char_p, other
    pointers -> c_void_p, scalars by value."""
    words = [t for t in tokens if t not in ("const", "*")]
    for t in words:
        if t not in _WORDS and t not in structs:
            raise ValueError(f"{where}: unknown type token {t!r}")
    base, stars = " ".join(words), tokens.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structs and base in _BYREF_STRUCTS:
        return POINTER(structs[base])
    if stars == 1 and base == "char" and "const" in tokens:
        return c_char_p
    if stars >= 1 and (base in _POINTEES or base in structs):
        return c_void_p
    raise ValueError(f"{where}: unsupported type {' '.join(tokens)!r}")


def _named(tokens, structs, where):
    """(name, ctypes type) of a `type name` declarator given as tokens"""
    if len(tokens) < 2 or not re.fullmatch(r"[A-Za-z_]\w*", tokens[-1]) or tokens[-1] in _WORDS | {"const"} or tokens[-1] in structs:
        raise ValueError(f"{where}: no type or no name in {' '.join(tokens)!r}")
    return tokens[-1], _ctype(tokens[:-1], structs, f"{where} {tokens[-1]}")


def parse_header(text):
    """C header text -> (constants {NAME: int}, structs {dei2i_x: Structure}, signatures {dei2i_f: (restype, argtypes)})"""
    tokens = re.compile(r"\w+|\S").findall
    constants, structs, signatures = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+DEI2I_(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        if not re.fullmatch(r"-?\d+|\(-?\d+\)", value):
            raise ValueError(f"#define DEI2I_{name}: {value!r} is not an integer")
        constants[name] = int(value.strip("()"))
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|typedef\s+void\s*\*\s*dei2i_stream\s*;|^\s*\}\s*$', " ", text, flags=re.M)

    def struct(m):
        fields = []
        for decl in filter(None, map(str.strip, m[2].split(";"))):       # `type a, b, c` shares the first declarator's type
            first, *more = map(str.strip, decl.split(","))
            name, ctype = _named(tokens(first), structs, f"struct {m[1]} field")
            for extra in more:
                if not re.fullmatch(r"[A-Za-z_]\w*", extra):
                    raise ValueError(f"struct {m[1]} field {name}: unsupported declarator {extra!r}")
            fields += [(n, ctype) for n in [name] + more]
        structs[m[1]] = type(m[1], (Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    *decls, tail = text.split(";")
    if tail.strip():
        raise ValueError(f"expected ';' after {tail.split()[-1]!r} at the end of the header")
    for decl in filter(str.strip, decls):
        m = re.match(r"\s*([\w\s*]+?)\b(dei2i_\w+)\s*\(([^()]*)\)\s*", decl)
        if not m or m.end() != len(decl):
            raise ValueError(f"{m[2] if m else 'header'}: expected ';' before {(decl[m.end():] if m else decl).split()[0]!r}")
        params = [] if m[3].strip() in ("", "void") else m[3].split(",")
        res = None if tokens(m[1]) == ["void"] else _ctype(tokens(m[1]), structs, f"{m[2]} return type")
        signatures[m[2]] = (res, [_named(tokens(p), structs, f"{m[2]} parameter")[1] for p in params])
    return constants, structs, signatures


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"the C ABI header {HEADER_PATH} is missing: the ctypes binding is derived from it")
with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, SIGNATURES = parse_header(_f.read())
globals().update(CONSTANTS)          # BF16, ACT_*, PAD_*, ERR_*, DIFFAUG_*, BLIT_*, WARP_*, PROF_*, EMBED_MAX_LABEL_NC, DIGEST_MAX_ROWS
ConvDesc, ProDesc, EpiNormDesc, LabelMod, AdamRec, DiffAugRec = (
    STRUCTS["dei2i_" + n] for n in ("conv", "pro", "epi_norm", "label_mod", "adam_rec", "diffaug_rec"))
ADAM_REC_WORDS = ctypes.sizeof(AdamRec) // 8          # int64 words in one row of a device table of dei2i_adam_rec

_lib = None


def load():
    """Load (once) and return the ctypes handle.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7; whichever copy is mapped first serves the whole process.  Import torch
    # first so this library shares torch's HIP runtime (streams, device pointers) instead of /opt/rocm's copy.
    import torch  # noqa: F401
    path = os.environ.get("DEI2I_LIB", LIB_PATH)     # a differently built copy of the SAME library, for same-box A/B timing
    if not os.path.exists(path):
        raise RuntimeError(
            f"libdei2i_hip.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU / PyTorch fallback for the de-i2i-gan_amd ops.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def launch_counts(reset=False):
    """{kernel family name: host-side launch count since the last reset} of the MFMA kernels (dei2i_launch_counts)."""
    lib = load()
    buf = (c_int64 * 32)()
    n = lib.dei2i_launch_counts(buf, 32)
    out = {lib.dei2i_kernel_name(i).decode(): int(buf[i]) for i in range(n)}
    if reset:
        lib.dei2i_launch_counts_reset()
    return out


def check(rc, what=""):
    if rc != 0:
        msg = load().dei2i_error_string(int(rc))
        raise RuntimeError(f"dei2i {what} failed: code {rc} ({msg.decode() if msg else '?'})")
