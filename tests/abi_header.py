"""include/raynet_hip.h as the tests read it: every prototype's return type and argument
declarations, and the ctypes type raynet_amd._lib's table must hold for each (no GPU, no compile).
One parser for tests/test_abi.py, which checks every entry, and for the stage tests, which pin the
literal prototypes of their own entries."""
import ctypes
import os
import re

from conftest import REPO

HEADER = os.path.join(REPO, "include", "raynet_hip.h")

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "double": ctypes.c_double}
# what a pointer in the table may point at; any other pointee only as c_void_p
POINTEES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
POINTED_AT_ONLY = ("void", "rn_ctx", "uint8_t", "uint64_t")
STRUCTS = {"rn_config": "Config", "rn_options": "Options", "rn_scene_plan": "ScenePlan",
           "rn_sampling": "Sampling"}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p,
           "void": None}

_cache = {}


def prototypes(path=HEADER):
    """{name: (return type, [argument declarations])}, white space normalised, in the header's
    order.  A statement of the header that is neither a typedef nor a prototype of an rn_ name is
    an error."""
    if path in _cache:
        return _cache[path]
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"\btypedef\s+[^{};]*;", "", text)
    text = re.sub(r"\btypedef\s+\w+\s*\{[^}]*\}\s*\w+\s*;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    found = {}
    for statement in text.split(";"):
        statement = " ".join(statement.split())
        if statement in ("", "}"):
            continue
        m = re.match(r"^(\w[\w ]*?\*?) ?\b(rn_\w+) ?\(([^()]*)\)$", statement)
        if m is None or m.group(2) in found:
            raise ValueError("%s: not a prototype the tests can read: %r" % (path, statement))
        arguments = [a.strip() for a in m.group(3).split(",")]
        found[m.group(2)] = (m.group(1).strip(), [] if arguments == ["void"] else arguments)
    _cache[path] = found
    return found


def prototype(name):
    """(return type, [argument declarations]) of one entry."""
    found = prototypes()
    assert name in found, "%s is not declared in include/raynet_hip.h" % name
    return found[name]


def restype_of(returns):
    """The restype the loaded function must have."""
    if returns not in RETURNS:
        raise ValueError("return type %r: unknown" % returns)
    return RETURNS[returns]


def argtype_of(declaration, bound=None):
    """The ctypes type the table must hold for one argument declaration.  A pointer or an array
    parameter is c_void_p -- or, where the table (`bound`) holds a typed pointer, that pointer if
    its pointee is the declared one."""
    from raynet_amd import _lib
    m = re.match(r"^(?:const )?(\w+) ?((?:\*(?: ?const)? ?)*)(\w+)((?:\[\d+\])?)$", declaration)
    if m is None:
        raise ValueError("argument %r: unknown form" % declaration)
    base, stars, array = m.group(1), m.group(2).count("*"), bool(m.group(4))
    if base in STRUCTS:
        if stars != 1 or array:
            raise ValueError("argument %r: a struct goes by one pointer" % declaration)
        return ctypes.POINTER(getattr(_lib, STRUCTS[base]))
    if base not in SCALARS and base not in POINTED_AT_ONLY:
        raise ValueError("argument %r: unknown type %r" % (declaration, base))
    depth = stars + (1 if array else 0)
    if depth == 0:
        if base not in SCALARS:
            raise ValueError("argument %r: %s by value" % (declaration, base))
        return SCALARS[base]
    pointee = ctypes.c_void_p if depth > 1 else POINTEES.get(base)
    if pointee is not None and bound is ctypes.POINTER(pointee):
        return bound
    return ctypes.c_void_p
