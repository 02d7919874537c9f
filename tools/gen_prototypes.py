#!/usr/bin/env python3
"""Write ``rasterizer/cuda/_prototypes.py`` from ``include/gsraster.h``.

Run it after declaring, removing or changing an entry in the header: ``python tools/gen_prototypes.py``
(tests/test_native_prototypes_host.py fails while the committed table is stale).

The table is data only: per entry, in header order, one letter for the return kind and one per parameter
(``KINDS`` below; ``rasterizer.cuda._backend`` maps them to ctypes).  The header is regular C: every entry is
``<type> gsr_name(<type> [name], ...);``, no struct is passed by value, and every pointer -- ``T *``, ``void *``,
``gsr_stream_t`` -- is one kind.  Anything else stops the generator instead of being guessed at.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsraster.h")
OUTPUT = os.path.join(ROOT, "gaussian-splatting-toolkit_amd", "rasterizer", "cuda", "_prototypes.py")

# scalar C types -> kind letter ("p": any pointer; "s", returns only: const char *)
KINDS = {"int": "i", "unsigned": "I", "unsigned int": "I", "float": "f", "double": "d", "size_t": "z",
         "long long": "q", "unsigned long long": "Q"}
POINTER_TYPEDEFS = ("gsr_stream_t",)


def _kind(decl: str, entry: str, is_return: bool = False) -> str:
    """``decl``: a parameter with or without its name, or a return type."""
    decl = " ".join(decl.split())
    if is_return and re.fullmatch(r"const char ?\*", decl):
        return "s"
    if "*" in decl or "[" in decl or decl.split()[0] in POINTER_TYPEDEFS:
        if is_return:
            raise ValueError(f"{entry}: return type {decl!r} is not one the bindings know")
        return "p"
    words = [w for w in decl.split() if w != "const"]
    # the longest leading run of words that names a scalar type; what follows is the parameter's name (at most one word)
    for k in range(len(words), 0, -1):
        kind = KINDS.get(" ".join(words[:k]))
        if kind is not None and len(words) - k <= (0 if is_return else 1):
            return kind
    raise ValueError(f"{entry}: cannot classify {decl!r} (a struct by value? add the type to KINDS)")


def parse(text: str):
    """-> [(name, return kind, parameter kinds)] in header order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)  # preprocessor lines, with continuations
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)
    text = re.sub(r"\btypedef\b[^;{]*;", " ", text)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", text)
    out = []
    for stmt in text.split(";"):
        stmt = " ".join(stmt.replace("}", " ").split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\b(gsr_[a-z0-9_]+) ?\((.*)\)", stmt)
        if m is None:
            raise ValueError(f"not a declaration of an entry: {stmt[:80]!r}")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if "(" in params:
            raise ValueError(f"{name}: function-pointer parameters are not supported")
        kinds = "" if params in ("", "void") else "".join(_kind(p, name) for p in params.split(","))
        out.append((name, _kind(ret, name, is_return=True), kinds))
    names = [n for n, _, _ in out]
    if len(set(names)) != len(names):
        raise ValueError("an entry is declared twice")
    return out


def render(entries) -> str:
    lines = ['"""Prototypes of the C ABI: generated from include/gsraster.h by tools/gen_prototypes.py -- do not edit.',
             "",
             "name: (return kind, one kind per parameter).  p pointer, i int, I unsigned, f float, d double, z size_t,",
             'q long long, Q unsigned long long, s const char * (``rasterizer.cuda._backend`` maps them to ctypes)."""',
             "PROTOTYPES = {"]
    lines += [f'    "{name}": ("{ret}", "{kinds}"),' for name, ret, kinds in entries]
    lines += ["}", ""]
    return "\n".join(lines)


def generate(header: str = HEADER) -> str:
    with open(header) as f:
        return render(parse(f.read()))


if __name__ == "__main__":
    text = generate()
    with open(OUTPUT, "w") as f:
        f.write(text)
    print(f"{OUTPUT}: {text.count('gsr_')} entries")
