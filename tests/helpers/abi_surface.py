"""What include/ptudes_mi.h declares and what a built library exports: the two sets a surface test holds against each other."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "ptudes_mi.h")


def header_text():
    """the header without comments"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def declared():
    """names of the functions the header declares"""
    src = re.sub(r"#define[^\n]*", " ", header_text())
    return set(re.findall(r"^[ \t]*(?:const\s+)?[A-Za-z_]\w*[\s\*]+(ptl_\w+)\s*\(", src, flags=re.M))


def exported(path):
    """names of the ptl_ functions a shared library defines"""
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("nm (binutils) is needed to list the library's exported symbols")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ptl_") and " T " in ln}


def struct_fields(name):
    """[(field, C type text, array length or None)] of a `typedef struct { ... } name;` of the header"""
    src = header_text()
    body = re.search(r"typedef struct \{([^}]*)\} " + name + r";", src).group(1)
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PTL_\w+) (\d+)\b", src)}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for f in rest.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", f.strip())
            out.append((m.group(1), ctype, None if m.group(2) is None else macros.get(m.group(2)) or int(m.group(2))))
    return out
