"""Shared by the tests of the Fortran and ctypes bindings: a parser of the prototypes of include/ohxgb.h, a parser of the
bind(C) interface blocks of quickchem_amd/fortran/ohx_bindings.F90, and the comparison of a block, or of a ctypes
argtypes list, with its prototype.  Both parsers take text, so that a test can hand them a changed copy.  Whatever
they cannot classify raises Unparsed: a test fails, it never skips.

The comparison is the table of tests/test_bindings_abi_cpu.py's docstring, written out in `compare_block` and
`compare_ctypes`; each returns a list of sentences, empty when the two sides agree."""
import ctypes as C
import re
from collections import namedtuple


class Unparsed(Exception):
    pass


# ---- the header ----

# base type -> (kind, bytes); kind is int, uint, float, char, void or struct
C_BASE = {"int": ("int", 4), "unsigned": ("uint", 4), "int32_t": ("int", 4), "uint32_t": ("uint", 4),
          "int64_t": ("int", 8), "uint64_t": ("uint", 8), "bst_ulong": ("uint", 8), "float": ("float", 4),
          "double": ("float", 8), "char": ("char", 1), "void": ("void", 0), "OHXRun1Args": ("struct", 0)}
# opaque handles: void* under another name
C_HANDLES = ("BoosterHandle", "DMatrixHandle", "OHXCommHandle")

CType = namedtuple("CType", "kind width depth")            # depth: pointer levels; 0 = by value
CParam = namedtuple("CParam", "type name")
CProto = namedtuple("CProto", "name ret params")


def _c_type(words, stars, where):
    words = [w for w in words if w != "const"]
    if len(words) != 1:
        raise Unparsed(f"{where}: type {' '.join(words)!r}")
    base = words[0]
    if base in C_HANDLES:
        base, stars = "void", stars + 1
    if base not in C_BASE:
        raise Unparsed(f"{where}: unknown type {base!r}")
    kind, width = C_BASE[base]
    if stars == 0 and kind in ("void", "struct", "char"):
        raise Unparsed(f"{where}: {base} by value")
    return CType(kind, width, stars)


def _c_param(text, where):
    m = re.fullmatch(r"(.*?)(\w+)\s*(\[\s*\d*\s*\])?", text.strip(), flags=re.S)
    if not m:
        raise Unparsed(f"{where}: parameter {text!r}")
    decl, name, array = m.groups()
    stars = decl.count("*") + (1 if array else 0)              # `T name[]` is one more pointer level
    return CParam(_c_type(decl.replace("*", " ").split(), stars, f"{where}, {name}"), name)


def parse_header(text):
    """-> {name: CProto} of every prototype, in the order of the text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"typedef\s+struct\b.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef\b[^;{}]*;", " ", text)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):                                  # the brace that closes extern "C"
            continue
        m = re.fullmatch(r"(.*?)(\w+)\s*\((.*)\)", stmt)
        if not m:
            raise Unparsed(f"not a prototype: {stmt[:80]!r}")
        ret, name, params = m.groups()
        ret = _c_type(ret.replace("*", " ").split(), ret.count("*"), f"{name}, return type")
        params = [] if params.strip() in ("", "void") else [_c_param(p, name) for p in params.split(",")]
        if name in protos:
            raise Unparsed(f"{name} is declared twice")
        protos[name] = CProto(name, ret, params)
    return protos


# ---- the Fortran text ----

FDummy = namedtuple("FDummy", "name type kind value array")   # type: integer, real, character or type
FBlock = namedtuple("FBlock", "name bind result dummies")     # result: an FDummy


def fortran_lines(text):
    """Statements of free-form source: `!` comments stripped (outside quotes), `&` continuations joined."""
    out, pending = [], ""
    for raw in text.split("\n"):
        line, quote = "", None
        for ch in raw:
            if quote:
                quote = None if ch == quote else quote
            elif ch in "'\"":
                quote = ch
            elif ch == "!":
                break
            line += ch
        line = line.strip()
        if pending and line.startswith("&"):
            line = line[1:].lstrip()
        if line.endswith("&"):
            pending += line[:-1] + " "
            continue
        if pending or line:
            out.append(pending + line)
        pending = ""
    if pending:
        raise Unparsed("the text ends in a continuation")
    return out


def _split_top(text):
    """Split at the commas that are not inside parentheses."""
    parts, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


_FUNCTION = re.compile(r'function\s+(\w+)\s*\(([^)]*)\)\s*bind\s*\(\s*C\s*,\s*name\s*=\s*"(\w+)"\s*\)\s*result\s*\(\s*(\w+)\s*\)',
                       re.I)
_DECL = re.compile(r"(integer|real|character|type)\s*\(\s*(?:kind\s*=\s*)?(\w+)\s*\)\s*(.*?)::\s*(.*)", re.I)


def parse_bindings(text):
    """-> {Fortran function name: FBlock} of every `function ... bind(C, name="...") result(..)` block."""
    blocks, lines, i = {}, fortran_lines(text), 0
    while i < len(lines):
        m = _FUNCTION.fullmatch(lines[i])
        if not m:
            if re.search(r"\bbind\s*\(\s*C\b", lines[i], re.I):
                raise Unparsed(f"a bind(C) statement of another form: {lines[i][:80]!r}")
            i += 1
            continue
        fname, dummy_list, bind, result = m.groups()
        order = [d.strip().lower() for d in dummy_list.split(",") if d.strip()]
        declared = {}
        i += 1
        while i < len(lines) and not re.fullmatch(r"end\s*function(\s+\w+)?", lines[i], re.I):
            stmt = lines[i]
            i += 1
            if re.match(r"import\b", stmt, re.I):
                continue
            d = _DECL.fullmatch(stmt)
            if not d:
                raise Unparsed(f"{fname}: statement {stmt!r}")
            ftype, kind, attrs, entities = d.groups()
            attrs = [a.strip().lower() for a in _split_top(attrs) if a.strip()]
            for a in attrs:
                if a != "value" and not re.fullmatch(r"intent\s*\(\s*(in|out|inout)\s*\)|dimension\s*\(.*\)|target", a):
                    raise Unparsed(f"{fname}: attribute {a!r}")
            for ent in _split_top(entities):
                e = re.fullmatch(r"(\w+)\s*(\(.*\))?", ent)
                if not e:
                    raise Unparsed(f"{fname}: entity {ent!r}")
                name = e.group(1).lower()
                if name in declared:
                    raise Unparsed(f"{fname}: {name} is declared twice")
                declared[name] = FDummy(name, ftype.lower(), kind.lower(), "value" in attrs,
                                        bool(e.group(2)) or any(a.startswith("dimension") for a in attrs))
        if i == len(lines):
            raise Unparsed(f"{fname}: no end function")
        i += 1
        if len(set(order)) != len(order):
            raise Unparsed(f"{fname}: a dummy occurs twice in the function statement")
        missing = [n for n in order + [result.lower()] if n not in declared]
        extra = [n for n in declared if n not in order and n != result.lower()]
        if missing or extra:
            raise Unparsed(f"{fname}: undeclared {missing}, declared but no dummy {extra}")
        if fname in blocks:
            raise Unparsed(f"{fname} has two blocks")
        blocks[fname] = FBlock(fname, bind, declared[result.lower()], [declared[n] for n in order])
    return blocks


# ---- a block against its prototype ----

def _pointee_matches(ct, d):
    """A non-value dummy against the pointee of a T*: a scalar or an array of T."""
    if ct.kind == "float":
        return d.type == "real" and d.kind == {4: "c_float", 8: "c_double"}[ct.width]
    if ct.kind in ("int", "uint"):
        return d.type == "integer" and d.kind in {4: ("c_int", "c_int32_t"), 8: ("c_int64_t",)}[ct.width]
    if ct.kind == "char":
        return d.type == "character" and d.kind == "c_char"
    return False


def _position(ct, d, void_by_reference):
    """None, or why dummy d cannot stand for a C parameter of type ct."""
    said = f"{d.type}({d.kind}){', value' if d.value else ''}{' array' if d.array else ''}"
    if ct.depth == 0:
        if d.array or not d.value:
            return f"a C scalar by value needs a scalar dummy with `value`, not {said}"
        if not _pointee_matches(ct, d):
            return f"C {ct.kind} of {ct.width} bytes by value, Fortran {said}"
        return None
    if d.type == "type":
        if d.kind != "c_ptr":
            return f"type({d.kind})"
        if d.value:
            return f"an array of pointers by value: {said}" if d.array else None      # any pointer, any handle
        # a c_ptr by reference is the address of a pointer: right for T** and for a handle by reference only
        return None if ct.depth >= 2 else f"a T* needs type(c_ptr) WITH value or a dummy of T, not {said}"
    if d.value:
        return f"a pointer needs type(c_ptr), value or a dummy by reference, not {said}"
    if ct.depth >= 2:
        return f"a T** needs type(c_ptr), not {said}"
    if ct.kind == "void":
        return None if void_by_reference and d.type == "character" and d.kind == "c_char" else \
            f"void* by reference ({said}) is allowed for the communicator id only"
    if not _pointee_matches(ct, d):
        return f"C pointer to {ct.kind} of {ct.width} bytes, Fortran {said}"
    return None


def compare_block(block, proto, renamed=(), void_by_reference=()):
    """renamed: {(block name, dummy name): header parameter name} for the dummies that go by another name;
    void_by_reference: (block name, dummy name) pairs.  -> a list of disagreements."""
    out = []
    if len(block.dummies) != len(proto.params):
        return [f"{block.name}: {len(block.dummies)} dummies, the header has {len(proto.params)} parameters"]
    for n, (d, p) in enumerate(zip(block.dummies, proto.params)):
        want = dict(renamed).get((block.name, d.name), d.name)
        if want.lower() != p.name.lower():
            out.append(f"{block.name}, position {n + 1}: dummy {d.name}, the header has {p.name}")
        why = _position(p.type, d, (block.name, d.name) in void_by_reference)
        if why:
            out.append(f"{block.name}, position {n + 1} ({p.name}): {why}")
    r, ct = block.result, proto.ret
    if r.value or r.array:
        out.append(f"{block.name}: a result with value or a shape")
    elif ct.depth == 0:
        if not _pointee_matches(ct, r):
            out.append(f"{block.name}: the result is {r.type}({r.kind}), the header returns {ct.kind} of {ct.width} bytes")
    elif not (r.type == "type" and r.kind == "c_ptr"):
        out.append(f"{block.name}: the header returns a pointer, the result is {r.type}({r.kind})")
    return out


# ---- a ctypes signature against its prototype ----

def _ctypes_scalar(t):
    """(kind, bytes) of a ctypes simple type that is a number, else None."""
    code = getattr(t, "_type_", None)
    if not isinstance(code, str):
        return None
    if code in "bhilq":
        return "int", C.sizeof(t)
    if code in "BHILQ":
        return "uint", C.sizeof(t)
    if code in "fd":
        return "float", C.sizeof(t)
    if code == "c":
        return "char", 1
    return None


def _ctypes_pointer(t, ct):
    """None, or why the ctypes type t cannot stand for a C pointer type ct (depth >= 1)."""
    if t is C.c_void_p:
        return None                                              # an address: any pointer
    if t is C.c_char_p:
        return None if (ct.kind, ct.depth) == ("char", 1) else f"c_char_p for a pointer to {ct.kind}, depth {ct.depth}"
    if not (isinstance(t, type) and issubclass(t, C._Pointer)):
        return f"{getattr(t, '__name__', t)} is no pointer type"
    inner = t._type_
    if ct.depth >= 2:
        return _ctypes_pointer(inner, ct._replace(depth=ct.depth - 1))
    if ct.kind == "struct":
        return None if issubclass(inner, C.Structure) else f"POINTER({inner.__name__}) for a pointer to a struct"
    if _ctypes_scalar(inner) != (ct.kind, ct.width):
        return f"POINTER({inner.__name__}) for a pointer to {ct.kind} of {ct.width} bytes"
    return None


def _ctypes_one(t, ct):
    if ct.depth == 0:
        got = _ctypes_scalar(t) if isinstance(t, type) else None
        return None if got == (ct.kind, ct.width) else \
            f"{getattr(t, '__name__', t)} for C {ct.kind} of {ct.width} bytes by value"
    return _ctypes_pointer(t, ct)


def compare_ctypes(name, argtypes, restype, proto):
    """-> a list of disagreements between a ctypes function's argtypes / restype and the prototype."""
    if argtypes is None:
        return [f"{name}: no argtypes"]
    if len(argtypes) != len(proto.params):
        return [f"{name}: {len(argtypes)} argtypes, the header has {len(proto.params)} parameters"]
    out = []
    for n, (t, p) in enumerate(zip(argtypes, proto.params)):
        why = _ctypes_one(t, p.type)
        if why:
            out.append(f"{name}, position {n + 1} ({p.name}): {why}")
    why = _ctypes_one(restype, proto.ret)
    if why:
        out.append(f"{name}, restype: {why}")
    return out


# ---- changed copies of the bindings text ----

def block_span(text, fname):
    """(start, end) of the block of function `fname` in the raw text: its function statement to its end function."""
    m = re.search(r"^[ \t]*function\s+" + re.escape(fname) + r"\s*\(", text, flags=re.M | re.I)
    if not m:
        raise Unparsed(f"no block {fname}")
    e = re.compile(r"^[ \t]*end\s*function\b.*$", flags=re.M | re.I).search(text, m.end())
    return m.start(), e.end()


def edit_block(text, fname, pattern, repl):
    """The text with ONE regex substitution made inside the block of `fname`; raises unless exactly one is made."""
    a, b = block_span(text, fname)
    new, n = re.subn(pattern, repl, text[a:b], flags=re.S)
    if n != 1 or new == text[a:b]:
        raise Unparsed(f"{fname}: {n} substitutions of {pattern!r}")
    return text[:a] + new + text[b:]
