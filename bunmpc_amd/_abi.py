"""Reader of include/bunmpc.h: the prototypes, structs and constants of the C-ABI as ctypes, so that bunmpc_amd/_lib.py declares
nothing a second time.  Pure Python; it reads the C subset that header uses and nothing else:

  * /* */ and // comments; preprocessor lines: #define NAME <number> is kept, an empty #define, #ifndef and #endif are dropped, an
    #ifdef __cplusplus ... #endif block (the extern "C" { wrapper and its brace) is skipped, anything else raises;
  * typedef struct X X_t;              an opaque handle, usable behind a pointer only;
  * typedef struct { ... } name_t;     fields of int, long, double, unsigned, char, pointers, 1-D and 2-D arrays, several declarators
                                       per declaration (unsigned grid, block;), several declarations per line, earlier structs by value;
  * res name(void); res name(params);  array parameters are pointers, parameter names are optional, const may stand anywhere.

Types map as ctypes callers expect: char * is c_char_p, every other pointer c_void_p, char x[N] is c_char * N.  Nothing is skipped
silently: a top-level statement or a struct member outside the subset, a type that is not known, and a struct or handle used before
its definition raise HeaderError with the statement in the message."""
import collections
import ctypes as C
import re

SCALARS = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "unsigned": C.c_uint, "char": C.c_char}

Abi = collections.namedtuple("Abi", "functions structs defines")      # {name: (restype, [argtypes])}, {C name: class}, {name: number}


class HeaderError(ValueError):
    pass


_DIMS = r"((?:\[\s*\d*\s*\])*)"
_MEMBER = re.compile(r"(\**)\s*(\w+)\s*" + _DIMS)
_PARAM = re.compile(r"(\w+)\s*(\**)\s*(\w+)?\s*" + _DIMS)
_PROTOTYPE = re.compile(r"(\w+)\s*(\**)\s*(\w+)\s*\((.*)\)")
_OPAQUE = re.compile(r"typedef struct (\w+) (\w+)")
_STRUCT = re.compile(r"typedef struct \{(.*)\} (\w+)")


def _preprocess(text):
    """(the C text without comments and preprocessor lines, {name: number} of its #defines)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    lines, defines, skipping = [], {}, False
    for line in text.split("\n"):
        word = line.split()
        if not line.lstrip().startswith("#"):
            if not skipping:
                lines.append(line)
        elif word[0] == "#endif":
            skipping = False
        elif word == ["#ifdef", "__cplusplus"]:
            skipping = True
        elif word[0] == "#define" and len(word) == 3 and "(" not in word[1]:
            try:
                defines[word[1]] = int(word[2], 0)
            except ValueError:
                try:
                    defines[word[1]] = float(word[2])
                except ValueError:
                    raise HeaderError("not a number: " + line.strip()) from None
        elif not (word[0] == "#ifndef" and len(word) == 2 or word[0] == "#define" and len(word) == 2):
            raise HeaderError("cannot read the preprocessor line: " + line.strip())
    return "\n".join(lines), defines


def _statements(text):
    """the top-level statements, each on one line with single spaces: split at the semicolons outside braces"""
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            out.append(" ".join(text[start:i].split()))
            start = i + 1
    if text[start:].strip() or depth:
        raise HeaderError("cannot read the end of the header: " + " ".join(text[start:].split())[:200])
    return out


def _ctype(base, pointer, dims, structs, opaque, where):
    """the ctypes type of `base`, behind a pointer or not, as an array of `dims` (outermost first)"""
    if base not in SCALARS and base not in structs and not (pointer and (base == "void" or base in opaque)):
        raise HeaderError("unknown type %r (a struct or handle must be defined before its use) in: %s" % (base, where))
    t = (C.c_char_p if base == "char" else C.c_void_p) if pointer else SCALARS.get(base) or structs[base]
    for n in reversed(dims):
        t = t * n
    return t


def _struct(name, body, structs, opaque, pyname):
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        base, _, rest = decl.partition(" ")
        for declarator in rest.split(","):
            m = _MEMBER.fullmatch(declarator.strip())
            if not m or m.group(2) in SCALARS:
                raise HeaderError("cannot read the member %r of %s" % (decl, name))
            dims = [int(n) for n in re.findall(r"\d+", m.group(3))]
            if len(dims) != m.group(3).count("["):
                raise HeaderError("array without a size: member %r of %s" % (decl, name))
            fields.append((m.group(2), _ctype(base, m.group(1), dims, structs, opaque, "%s { %s; }" % (name, decl))))
    return type(pyname, (C.Structure,), {"_fields_": fields, "__doc__": name})


def _prototype(stmt, structs, opaque):
    m = _PROTOTYPE.fullmatch(stmt)
    if not m or m.group(3) in SCALARS:
        raise HeaderError("cannot read the statement: " + stmt)
    res = None if (m.group(1), m.group(2)) == ("void", "") else _ctype(m.group(1), m.group(2), [], structs, opaque, stmt)
    args = []
    for param in ([] if m.group(4).strip() == "void" else m.group(4).split(",")):
        p = _PARAM.fullmatch(param.strip())
        if not p or p.group(3) in SCALARS or p.group(3) == "void":
            raise HeaderError("cannot read the parameter %r of: %s" % (param.strip(), stmt))
        args.append(_ctype(p.group(1), p.group(2) or p.group(4), [], structs, opaque, stmt))
    return m.group(3), (res, args)


def parse(text, names=None):
    """Abi of a header's text.  names: {C struct name: name of its ctypes class} (default: the C name)."""
    text, defines = _preprocess(text)
    functions, structs, opaque = {}, {}, set()
    for stmt in _statements(text):
        stmt = " ".join(re.sub(r"\bconst\b", " ", stmt).split())      # whole words: loop_constants_in_lds is a field
        if m := _OPAQUE.fullmatch(stmt):
            opaque.add(m.group(2))
        elif m := _STRUCT.fullmatch(stmt):
            structs[m.group(2)] = _struct(m.group(2), m.group(1), structs, opaque, (names or {}).get(m.group(2), m.group(2)))
        else:
            name, sig = _prototype(stmt, structs, opaque)
            functions[name] = sig
    return Abi(functions, structs, defines)


def read(path, names=None):
    with open(path) as f:
        return parse(f.read(), names)
