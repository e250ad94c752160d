"""Reader of the restricted C that include/stlpose_hip.h is written in: integer ``#define``s, ``typedef struct``s and prototypes
become Python ints, ``ctypes.Structure`` classes and argtypes / restypes.  No compiler and no preprocessor run: whatever is outside
that subset raises ``SyntaxError`` with its line, so a header edit the reader does not understand cannot drop a symbol quietly."""
import ctypes as C
import os
import re

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "uint8_t": C.c_uint8, "uint64_t": C.c_uint64}
POINTEES = ("void", "long long")   # besides the scalars and the structs: what appears only behind a pointer
RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}

_DEFINE = re.compile(r"#define\s+(STL_\w+)(\(.*?\))?\s+(.+)")
_GUARD = re.compile(r"#(ifndef \w+_H|define \w+_H|ifdef __cplusplus|endif|include <stdint\.h>)")
_SPACE = re.compile(r"\s*")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(int|int64_t|const char\*)\s+(stl_\w+)\s*\(([^()]*)\)\s*;")
_DECL = re.compile(r"(?:const\s+)?(long long|\w+)\s*((?:\*\s*(?:const\s*)?)*)\b(\w+)\s*(?:\[(\w+)\])?")
_MORE = re.compile(r"(\w+)\s*(?:\[(\w+)\])?")   # the later declarators of one member line: `int32_t B, Hi, wait[8];`


class Header:
    def __init__(self, path, class_names=None, device_records=(), base=None):
        """``class_names``: C struct name -> Python class name (default: the C name).  ``device_records``: the structs that live in
        device tables, so that a pointer to one is a raw address (``c_void_p``) and not ``POINTER(Class)``.  ``base``: the Header of
        the one file this header may ``#include "..."``: its structs (the same classes) and constants are known here, and
        ``structs`` / ``constants`` then hold them too."""
        self.path, self.class_names, self.device_records = path, class_names or {}, tuple(device_records)
        self.base = base
        self.constants = dict(base.constants) if base else {}   # "STL_NAME" -> int
        self.structs = dict(base.structs) if base else {}       # C name -> ctypes.Structure subclass, in header order
        if base:
            self.device_records += tuple(base.device_records)
        self.signatures, self.restypes = {}, {}    # function name -> argtypes list / restype
        with open(path) as f:   # comments go, their line breaks stay: errors name the header's own line
            text = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), f.read(), flags=re.S)
        self.lines = [line.strip() for line in text.split("\n")]
        code, cplusplus = [], False
        for n, s in enumerate(self.lines):
            if cplusplus or s.startswith("#"):
                cplusplus = self._directive(n, s, cplusplus)
                s = ""
            code.append(s)
        self._declarations("\n".join(code))

    def _fail(self, n, why="outside the C subset this reader knows"):
        raise SyntaxError(f"{self.path}:{n + 1}: {why}: {self.lines[n]!r}")

    def _directive(self, n, s, cplusplus):
        """One preprocessor line, or a line of the ``extern "C"`` block.  Returns whether the next line is inside that block."""
        if cplusplus:
            if s not in ('extern "C" {', "}", "#endif"):
                self._fail(n)
            return s != "#endif"
        m = _DEFINE.fullmatch(s)
        if m and not m.group(2):   # a macro with parameters (STL_DT2) is no constant
            if not re.fullmatch(r"[\d\s()<+*|-]+", m.group(3)):
                self._fail(n, "not an integer expression")
            self.constants[m.group(1)] = int(eval(m.group(3), {"__builtins__": {}}))
        elif not m and not _GUARD.fullmatch(s) and not (self.base and s == f'#include "{os.path.basename(self.base.path)}"'):
            self._fail(n)
        return s == "#ifdef __cplusplus"

    def _declarations(self, code):
        pos = _SPACE.match(code).end()
        while pos < len(code):
            n = code.count("\n", 0, pos)
            if m := _STRUCT.match(code, pos):
                fields = [f for line in m.group(1).split(";") if line.strip() for f in self._declare(n, line.split(","))]
                self.structs[m.group(2)] = type(self.class_names.get(m.group(2), m.group(2)), (C.Structure,), {"_fields_": fields})
            elif m := _PROTO.match(code, pos):
                params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
                self.signatures[m.group(2)] = [t for p in params for _, t in self._declare(n, [p])]
                self.restypes[m.group(2)] = RESTYPES[m.group(1)]
            else:
                self._fail(n)
            pos = _SPACE.match(code, m.end()).end()

    def _declare(self, n, declarators):
        """``[type name]`` of a parameter or ``[type a, b[4], c]`` of a struct member line -> [(name, ctype)]."""
        first, *more = [" ".join(d.split()) for d in declarators]
        m = _DECL.fullmatch(first)
        if not m or (more and m.group(2)):   # `float *a, b` gives b another type than a: not written in this header
            self._fail(n, f"cannot read the declaration {first!r}")
        base, stars = m.group(1), m.group(2).count("*")
        if base not in SCALARS and base not in self.structs and not (stars and base in POINTEES):
            self._fail(n, f"unknown type {base!r}")
        if stars:
            host = stars == 1 and base in self.structs and base not in self.device_records
            ctype = C.POINTER(self.structs[base]) if host else C.c_void_p
        else:
            ctype = SCALARS.get(base) or self.structs[base]
        out = []
        for name, extent in [m.group(3, 4)] + [(_MORE.fullmatch(d) or self._fail(n, f"cannot read {d!r}")).groups() for d in more]:
            if extent and not (extent.isdigit() or extent in self.constants):
                self._fail(n, f"unknown array extent {extent!r}")
            out.append((name, ctype * int(self.constants.get(extent, extent)) if extent else ctype))
        return out
