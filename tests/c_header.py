"""A reader for the two plain-C headers the ctypes bindings mirror (include/ptc.h, oracle/ptc_oracle.h): prototypes, structs, and integer constants,
each reduced to the classes a ctypes declaration can get wrong.  It knows the C these headers use and raises on anything else, so that a new construct
is noticed instead of skipped.

A value's class is one of "void", "ptr" (pointers and array parameters), "float", "double", "int8", "int16", "int32", "int64"."""
import ctypes as C
import re

_SCALARS = {"void": "void", "float": "float", "double": "double", "int": "int32", "int32_t": "int32", "uint32_t": "int32", "int64_t": "int64",
            "uint64_t": "int64", "uint16_t": "int16", "int16_t": "int16", "uint8_t": "int8", "int8_t": "int8"}


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _scalar(type_words, where):
    words = [w for w in type_words if w != "const"]
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError(f"{where}: type {' '.join(type_words)!r} is not one this reader knows")
    return _SCALARS[words[0]]


def _parameter(text, where):
    """(class, array length or None) of one parameter; its name, if it has one, is dropped."""
    m = re.search(r"\[\s*(\w*)\s*\]", text)
    if m or "*" in text:
        return "ptr", (m.group(1) or None) if m else None
    words = text.split()
    known = [w for w in words if w in _SCALARS]
    if len(known) != 1 or words.index(known[0]) > 1:
        raise ValueError(f"{where}: parameter {text!r} is not one this reader knows")
    return _scalar(words[:words.index(known[0]) + 1], where), None


class Header:
    def __init__(self, path, prefix):
        text = _strip(open(path).read())
        self.constants = {}
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(%s\w+)[ \t]+\(?(-?\w+)\)?[ \t]*$" % prefix.upper(), text, flags=re.M):
            self.constants[name] = int(value, 0)
        text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
        for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
            value = -1
            for entry in filter(None, (e.strip() for e in body.split(","))):
                name, _, expr = (s.strip() for s in entry.partition("="))
                value = self._int(expr) if expr else value + 1      # an implicit value counts on from the previous enumerator
                self.constants[name] = value
        # name -> (class of the result, [(class, array length) of each parameter])
        self.prototypes = {}
        for ret, name, params in re.findall(r"\b((?:const\s+)?\w+[\s*]+)(%s\w+)\s*\(([^()]*)\)\s*;" % prefix, text):
            assert name not in self.prototypes, f"{name} is declared twice"
            plist = [] if params.strip() in ("", "void") else [_parameter(p.strip(), name) for p in params.split(",")]
            self.prototypes[name] = ("ptr" if "*" in ret else _scalar(ret.split(), name), plist)
        # name -> [(field, class, array length or None)]; opaque handles (declared, never defined) are not here
        self.structs = {}
        for tag, body, name in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
            assert tag == name, f"struct {tag} is typedef'd as {name}"
            fields = []
            for decl in filter(None, (d.strip() for d in body.split(";"))):
                words = decl.replace(",", " , ").split()
                kind = _scalar(words[:1], name)
                for d in "".join(words[1:]).split(","):
                    m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", d)
                    if not m:
                        raise ValueError(f"{name}: declarator {d!r} is not one this reader knows")
                    fields.append((m.group(1), kind, self._int(m.group(2)) if m.group(2) else None))
            self.structs[name] = fields

    def _int(self, expr):
        expr = expr.strip("() \t\n")
        return self.constants[expr] if expr in self.constants else int(expr, 0)

    def array_length(self, function, index):
        """The declared length of array parameter `index` of `function` (a number, or a constant of this header)."""
        return self._int(self.prototypes[function][1][index][1])


def ctype_class(t):
    """The class of a ctypes restype / argtype / field type, in the header's terms."""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "ptr"
    if t in (C.c_float, C.c_double):
        return "float" if t is C.c_float else "double"
    if issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ":
        return f"int{8 * C.sizeof(t)}"
    raise ValueError(f"{t} is not a type this reader knows")


def mirror_name(struct):
    """ptc_lens_params -> PtcLensParams."""
    return "".join(w.capitalize() for w in struct.split("_"))


def check_prototypes(header, table):
    """The differences between a binding's name -> (restype, argtypes) table and the header's prototypes, as a list of sentences."""
    bad = [f"{n}: in the table, not in the header" for n in table if n not in header.prototypes]
    for name, (ret, params) in header.prototypes.items():
        if name not in table:
            bad.append(f"{name}: in the header, not in the table")
            continue
        restype, argtypes = table[name]
        if ctype_class(restype) != ret:
            bad.append(f"{name}: returns {ret}, the table says {ctype_class(restype)}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: takes {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for k, (t, (kind, _)) in enumerate(zip(argtypes, params)):
            if ctype_class(t) != kind:
                bad.append(f"{name}: parameter {k} is {kind}, the table says {ctype_class(t)}")
    return bad


def check_struct(fields, mirror):
    """The differences between a header struct's fields and a ctypes.Structure mirror."""
    got = [(k, ctype_class(t._type_), t._length_) if issubclass(t, C.Array) else (k, ctype_class(t), None) for k, t in mirror._fields_]
    return [] if got == fields else [f"{mirror.__name__}: the header has {fields}, the mirror {got}"]
