"""include/orbfe.h as data: constants, record structs and prototypes, parsed from the header's own text.

The parser knows exactly the C subset the header is written in -- integer `#define`s, anonymous enums, scalar typedefs, opaque
handles, `typedef struct NAME { ... } NAME;` records of scalars, pointers, fixed arrays and earlier records, and prototypes of
such types -- and raises HeaderError, naming the declaration, on anything else: nothing is skipped."""
import ctypes as C
import re

import numpy as np

SCALARS = {"float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
# [const] BASE, then the declarator: stars, an optional name, array bounds
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*((?:\[\w+\]\s*)*)$")
_FIELD = re.compile(r"((?:\*\s*(?:const\s*)?)*)(\w+)\s*((?:\[\w+\]\s*)*)$")


class HeaderError(ValueError):
    pass


class Header:
    """constants: {name: int} (also attributes: header.ORBFE_TH_HIGH); structs: {C name: ctypes.Structure class}; opaque: handle
    type names; prototypes: {name: (restype, argtypes)}.  A pointer to a struct named in `byref` is POINTER of its class, `const
    char *` is c_char_p, every other pointer (arrays, T **, handles) c_void_p."""

    def __init__(self, text, byref=()):
        self.constants, self.structs, self.opaque, self.prototypes = {}, {}, set(), {}
        self.scalars, self.byref = dict(SCALARS), tuple(byref)
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r'#ifdef __cplusplus\s*(?:extern "C" \{|\})\s*#endif', "", text)
        text = re.sub(r"^[ \t]*#[^\n]*$", self._directive, text, flags=re.M)
        text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", self._enum, text)
        text = re.sub(r"\btypedef struct (\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", self._record, text)
        for decl in text.split(";"):
            if decl.strip():
                self._declaration(" ".join(decl.split()))
        for name in self.byref:
            if name not in self.structs:
                raise HeaderError(f"no struct {name} to pass by reference")

    def __getattr__(self, name):
        try:
            return self.__dict__["constants"][name]
        except KeyError:
            raise AttributeError(name) from None

    def _int(self, tok, where):
        if re.fullmatch(_INT, tok):
            return int(tok, 0)
        if tok in self.constants:
            return self.constants[tok]
        raise HeaderError(f"{where}: {tok!r} is neither an integer nor a known constant")

    def _directive(self, m):
        line = " ".join(m.group(0).split())
        d = re.fullmatch(rf"#define (\w+) ({_INT})", line)
        if d:
            self.constants[d.group(1)] = int(d.group(2), 0)
        elif not re.fullmatch(r"#(include <\w+\.h>|ifndef \w+_H|define \w+_H|endif)", line):
            raise HeaderError(f"unsupported preprocessor line: {line}")
        return ""

    def _enum(self, m):
        value = -1
        for item in filter(None, (" ".join(i.split()) for i in m.group(1).split(","))):
            e = re.fullmatch(r"(\w+)(?: = (\S+))?", item)
            if not e:
                raise HeaderError(f"unsupported enumerator: {item}")
            value = value + 1 if e.group(2) is None else self._int(e.group(2), e.group(1))
            self.constants[e.group(1)] = value
        return ""

    def _record(self, m):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise HeaderError(f"struct {name}: typedef'd as {m.group(3)}")
        for decl in filter(None, (" ".join(d.split()) for d in m.group(2).split(";"))):
            self._members(name, decl, fields)
        self.structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        return ""

    def _members(self, name, decl, fields):
        m = re.fullmatch(r"(?:const )?(\w+) (.+)", decl)
        if not m:
            raise HeaderError(f"struct {name}: unsupported member {decl!r}")
        for d in m.group(2).split(","):
            f = _FIELD.fullmatch(d.strip())
            if not f:
                raise HeaderError(f"struct {name}: unsupported member {decl!r}")
            ctype = self._ctype(m.group(1), f.group(1), f"struct {name}: {decl!r}", member=True)
            for bound in reversed(re.findall(r"\w+", f.group(3))):
                ctype = ctype * self._int(bound, f"struct {name}: {decl!r}")
            fields.append((f.group(2), ctype))

    def _ctype(self, base, stars, where, member=False):
        nstars = stars.count("*")
        if base not in self.scalars and base not in self.structs and not (nstars and (base in self.opaque or base in ("void", "char"))):
            raise HeaderError(f"{where}: unknown type {base!r}")
        if nstars == 0:
            if base in self.scalars:
                return self.scalars[base]
            if member:
                return self.structs[base]
            raise HeaderError(f"{where}: {base} passed by value")
        if member or nstars > 1:
            return C.c_void_p
        if base == "char":
            return C.c_char_p
        return C.POINTER(self.structs[base]) if base in self.byref else C.c_void_p

    def _declaration(self, decl):
        m = re.fullmatch(r"typedef (?:struct )?(\w+) (\w+)", decl)
        if m:   # `typedef struct orbfe_handle orbfe_handle;` or `typedef int32_t orbfe_status;`
            if decl.startswith("typedef struct") and m.group(1) == m.group(2):
                self.opaque.add(m.group(2))
            elif not decl.startswith("typedef struct") and m.group(1) in self.scalars:
                self.scalars[m.group(2)] = self.scalars[m.group(1)]
            else:
                raise HeaderError(f"unsupported typedef: {decl}")
            return
        m = re.fullmatch(r"(?:const )?(\w+) ?(\**) ?(\w+) ?\((.*)\)", decl)
        if not m:
            raise HeaderError(f"unsupported declaration: {decl}")
        base, stars, name, params = m.groups()
        restype = None if (base, stars) == ("void", "") else self._ctype(base, stars, name)
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            d = _DECL.fullmatch(p.strip())
            if not d:
                raise HeaderError(f"{name}: unsupported parameter {p.strip()!r}")
            for bound in re.findall(r"\w+", d.group(4)):
                self._int(bound, f"{name}: {p.strip()!r}")
            argtypes.append(self._ctype(d.group(1), d.group(2) + "*" * bool(d.group(4)), f"{name}: {p.strip()!r}"))
        self.prototypes[name] = (restype, argtypes)

    def dtype(self, name, **shapes):
        """The numpy record dtype of struct `name`, laid out as the C compiler does.  A keyword reshapes an array member (same
        element count: T12=(4, 4)) or gives a nested record's dtype (same size)."""
        d = np.dtype(self.structs[name])
        formats = {n: d.fields[n][0] for n in d.names}
        for n, shape in shapes.items():
            new = shape if isinstance(shape, np.dtype) else np.dtype((formats[n].base, shape))
            if new.itemsize != formats[n].itemsize:
                raise ValueError(f"{name}.{n}: {shape} does not keep the member's size")
            formats[n] = new
        return np.dtype(dict(names=list(d.names), formats=[formats[n] for n in d.names], offsets=[d.fields[n][1] for n in d.names],
                             itemsize=d.itemsize))
