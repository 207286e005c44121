"""What the two ctypes-mirror tests share (test_abi_mirror.py: abi.PROTOTYPES against include/srt.h; test_host_abi_mirror.py:
host.PROTOTYPES against csrc/host/srt_host_c.h): the parser of a C header and the check of a prototype table against it."""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint8_t": C.c_uint8, "int32_t": C.c_int32,
           "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
RESTYPES = {**SCALARS, "void": None, "char*": C.c_char_p, "void*": C.c_void_p}


def _c_type(words):
    """'const float * const *' -> 'float**': const dropped, the stars joined to the base type."""
    t = re.sub(r"\bconst\b", " ", words)
    return "".join(t.replace("*", " ").split()) + "*" * t.count("*")


def parse_header(text, prefix="srt_"):
    """A C header as {"prototypes": [(name, return type, [(parameter type, parameter name)])] of the functions named prefix* in the
    header's order, "structs": {name: [field name]}, "constants": {name: value}}; types as _c_type writes them."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    value = lambda expr: eval(re.sub(r"\b(\d+)[uU]\b", r"\1", expr), {"__builtins__": {}})
    constants = {name: value(expr) for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SRT_\w+)[ \t]+([0-9][^\n]*)$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
        for entry in filter(None, (e.strip() for e in body.split(","))):
            name, expr = entry.split("=")
            constants[name.strip()] = value(expr)
    structs = {}
    for body, name in re.findall(r"\btypedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        structs[name] = [re.match(r"[\s\*]*(\w+)", d).group(1) for decl in filter(None, (re.sub(r"\bconst\b", "", d).strip() for d in body.split(";")))
                         for d in re.sub(r"^\w+", "", decl).split(",")]     # 'type a, *b, c[4]' -> a, b, c
    text = re.sub(r"\b(typedef\s+struct\s+\w+|enum)\s*\{.*?\}\s*\w*\s*;", " ", text, flags=re.S)
    prototypes = []
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(" + re.escape(prefix) + r"\w+)\s*\(([^()]*)\)\s*;", text):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.match(r"^(.*?)(\w+)\s*(\[\s*\d*\s*\])?$", p.strip())
            args.append((_c_type(m.group(1) + ("*" if m.group(3) else "")), m.group(2)))
        prototypes.append((name, _c_type(ret), args))
    return {"prototypes": prototypes, "structs": structs, "constants": constants}


def expected_argtype(function, c_type, parameter, structs):
    """The ctypes type the mirror's rule gives a parameter of include/srt.h."""
    if c_type.endswith("**"):                           # srt_scene**, T* const*: a table of addresses
        return C.POINTER(C.c_void_p)
    if c_type in ("srt_scene*", "void*"):
        return C.c_void_p
    if c_type.endswith("*"):
        base = c_type[:-1]
        if base.startswith("srt_"):
            return C.POINTER(structs[base])
        # an address that travels as an int: a device pointer, the pinned outputs of srt_render_async
        if parameter.startswith("d_") or function == "srt_render_async":
            return C.c_void_p
        return C.POINTER(SCALARS[base])
    return SCALARS[c_type]


def check_prototypes(table, structs, header, argtype=expected_argtype):
    """Every difference between the prototype table and the header's declarations, as 'function: what'."""
    declared = {name: (ret, args) for name, ret, args in header["prototypes"]}
    errors = [f"{name}: in the table, not in the header" for name in table if name not in declared]
    errors += [f"{name}: in the header, not in the table" for name in declared if name not in table]
    for name, (ret, args) in declared.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        if restype is not RESTYPES[ret]:
            errors.append(f"{name}: restype {restype} for '{ret}'")
        if len(argtypes) != len(args):
            errors.append(f"{name}: {len(argtypes)} argtypes for {len(args)} parameters")
            continue
        for i, ((c_type, parameter), have) in enumerate(zip(args, argtypes)):
            want = argtype(name, c_type, parameter, structs)
            if have is not want:
                errors.append(f"{name}: argument {i} ({c_type} {parameter}) is {have}, not {want}")
            if (parameter.startswith("d_") and c_type.count("*") == 1 or parameter == "stream") and have is not C.c_void_p:
                errors.append(f"{name}: {parameter} must be c_void_p")
    return errors
