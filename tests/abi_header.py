"""A C ABI header of include/ read without a compiler, and one record of doda_amd._lib.ABIS held to it (tests/test_abi_host.py).
A C type is written base + stars ("int32_t", "float*", "void**"); anything the reader does not know is an error, not a guess."""
import collections
import ctypes as C
import re

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
Header = collections.namedtuple("Header", "functions structs defines")   # name -> (return type, [argument types]) /
#                                                                           [(field, C type, array length or None)] / int
_DECL = r"(?:const\s+)?(?:struct\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*(?:\[(\d+)\])?"


def is_pointer(ctype):
    return ctype.endswith("*") or ctype == "doda_stream_t"


def to_ctypes(ctype):
    if is_pointer(ctype):
        return C.c_void_p
    if ctype not in SCALARS:
        raise ValueError("unknown C type %r" % ctype)
    return SCALARS[ctype]


def _declarations(text):
    """'const float *a, *b' -> [('a', 'float*', None), ('b', 'float*', None)]; 'int32_t dims[3]' -> [('dims', 'int32_t', 3)]"""
    first, *rest = [part.strip() for part in text.split(",")]
    m = re.fullmatch(_DECL, first)
    if not m:
        raise ValueError("cannot read the declaration %r" % text)
    out = [(m[3], m[1] + "*" * m[2].count("*"), int(m[4]) if m[4] else None)]
    for part in rest:
        r = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?", part)
        out.append((r[2], m[1] + "*" * len(r[1]), int(r[3]) if r[3] else None))
    return out


def int_expr(text):
    """Integers (a `u` suffix allowed), <<, parentheses and a unary minus; no eval."""
    toks = re.findall(r"0[xX][0-9a-fA-F]+[uU]?|\d+[uU]?|<<|\S", text)

    def unary():
        t = toks.pop(0)
        if t == "-":
            return -unary()
        if t == "(":
            v = shift()
            if toks.pop(0) != ")":
                raise ValueError(text)
            return v
        return int(t.rstrip("uU"), 0)

    def shift():
        v = unary()
        while toks and toks[0] == "<<":
            toks.pop(0)
            v <<= unary()
        return v
    try:
        v = shift()
        if toks:
            raise ValueError
    except (IndexError, ValueError):
        raise ValueError("not an integer expression: %r" % text) from None
    return v


def read_header(text):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int_expr(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DODA_\w+)[ \t]+(\S.*)$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        structs[m[2]] = [d for stmt in m[1].split(";") if stmt.strip() for d in _declarations(stmt)]
    functions = {}
    for stmt in re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", "", text).split(";"):
        stmt = stmt.strip().lstrip("}").strip()
        if not stmt or stmt.startswith("typedef"):
            continue
        m = re.fullmatch(r"([^()]+)\(([^()]*)\)", stmt)
        if not m:
            raise ValueError("cannot read the statement %r" % stmt)
        (name, ret, _), = _declarations(m[1])
        args = [] if m[2].strip() == "void" else [d[1] for a in m[2].split(",") for d in _declarations(a)]
        functions[name] = (ret, args)
    return Header(functions, structs, defines)


def _argument(ctype, got, structs):
    """None, or what is wrong with the table's type `got` for a header argument of type `ctype`."""
    if not is_pointer(ctype):
        return None if got is to_ctypes(ctype) else "header %s, table %s" % (ctype, got.__name__)
    if got in (C.c_void_p, C.c_char_p):
        return None
    if not (isinstance(got, type) and issubclass(got, C._Pointer)):
        return "header %s, table %s" % (ctype, getattr(got, "__name__", got))
    want = structs[ctype[:-1]] if ctype[:-1] in structs else to_ctypes(ctype[:-1])
    return None if got._type_ is want else "header %s, table POINTER(%s)" % (ctype, got._type_.__name__)


def compare(text, abi):
    """Every way the record `abi` differs from the header `text`, as 'kind name: what' lines; [] when they agree."""
    h, out = read_header(text), []
    for name in sorted(set(h.functions) ^ set(abi.signatures)):
        out.append("function %s: in the %s only" % (name, "header" if name in h.functions else "table"))
    for name in sorted(set(h.functions) & set(abi.signatures)):
        (ret, args), (res, argtypes) = h.functions[name], abi.signatures[name]
        want = {"void": None, "char*": C.c_char_p}[ret] if ret in ("void", "char*") else to_ctypes(ret)
        if res is not want:
            out.append("function %s: return type: header %s, table %s" % (name, ret, getattr(res, "__name__", res)))
        if len(args) != len(argtypes):
            out.append("function %s: argument count: header %d, table %d" % (name, len(args), len(argtypes)))
            continue
        for k, (ctype, got) in enumerate(zip(args, argtypes)):
            wrong = _argument(ctype, got, abi.structs)
            if wrong:
                out.append("function %s: argument %d: %s" % (name, k, wrong))
    for name in sorted((set(h.structs) - set(abi.unmirrored)) ^ set(abi.structs)):
        out.append("struct %s: in the %s only" % (name, "header" if name in h.structs else "record"))
    for name in sorted(set(h.structs) & set(abi.structs)):
        fields, mirror = h.structs[name], abi.structs[name]
        probe = type("Probe", (C.Structure,), {"_fields_": [(f, to_ctypes(t) * n if n else to_ctypes(t)) for f, t, n in fields]})
        if [f for f, _ in mirror._fields_] != [f for f, _, _ in fields]:
            out.append("struct %s: field names: header %s, mirror %s" % (name, [f for f, _, _ in fields], [f for f, _ in mirror._fields_]))
            continue
        for (f, t, _), (_, got) in zip(fields, mirror._fields_):
            a, b = getattr(probe, f), getattr(mirror, f)
            if (a.offset, a.size) != (b.offset, b.size) or not (is_pointer(t) or got is dict(probe._fields_)[f]):
                out.append("struct %s: field %s: header %s at %d (%d bytes), mirror %s at %d (%d bytes)"
                           % (name, f, t, a.offset, a.size, got.__name__, b.offset, b.size))
        if C.sizeof(probe) != C.sizeof(mirror):
            out.append("struct %s: sizeof: header %d, mirror %d" % (name, C.sizeof(probe), C.sizeof(mirror)))
    for name, value in [(abi.version_fn.upper()[5:], abi.version)] + sorted(abi.constants.items()):
        if h.defines.get("DODA_" + name) != value:
            out.append("constant %s: header %s, mirror %s" % (name, h.defines.get("DODA_" + name), value))
    return out
