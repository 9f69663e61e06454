#!/usr/bin/env python3
"""Instruction mix of one device function of the gfx950 code, and of each of its loops (host only, no GPU).

    python tools/isa_mix.py ptudes-lab_amd/csrc/libptudes_mi.so 'sq_gauss_newton<20,2>'
    python tools/isa_mix.py build/ptudes_mi-hip-amdgcn-amd-amdhsa-gfx950.s _Z10sq_preparePK6SeqCtxiiiijPjb --list div/sqrt --loop 3
    python tools/isa_mix.py LIB --symbols gauss          # the function names that contain "gauss"
    python tools/isa_mix.py LIB --notes kx_seq_run       # registers, spilled registers, scratch and LDS of the kernels named so

Input: the built library (the gfx950 code object is cut out of its fat binary and disassembled with the ROCm llvm-objdump) or the device
assembly a `hipcc --save-temps` build leaves (ptudes_mi-hip-amdgcn-amd-amdhsa-gfx950.s).  The function is named mangled, or demangled as
`name<template arguments>` (integers only), or by any substring that matches exactly one function.

Loops: in an assembly file the compiler's own comments delimit them - a header block says "Loop Header" with its depth and parents, every
other block names the header of its innermost loop; a disassembly carries no comments, so there the targets of backward branches stand
in for headers, each loop reaching to the last branch back (an approximation).  Every loop is printed with
the counts of its whole extent (nested loops included) and of what is its own (nested loops excluded): the own column of a loop is what one
trip through it executes at most, whatever its inner loops do.

Classes (static counts; what a lane executes depends on the branches):
  move        v_mov_*, v_accvgpr_*, v_swap_*                              register copies
  fp64        every other VALU instruction with an _f64 operand type      the arithmetic proper
  div/sqrt    v_div_scale / v_div_fmas / v_div_fixup / v_rcp / v_rsq / v_sqrt (any width): the frame of a division or square-root sequence
              (its FMAs count as fp64); "sequences" = v_div_fixup + v_rsq + v_sqrt
  self-max    v_max_* x, a, a: the canonicalisation the compiler puts in front of fmin / fmax
  lane        v_readlane / v_writelane: scalars kept in VGPR lanes (SGPR spills) and real cross-lane reads alike
  ctl         branches, exec-mask saves, scalar instructions that read or write exec
  vmem / lds / smem / wait (s_waitcnt, s_nop, s_barrier, s_sleep) / valu (other vector) / salu (other scalar)
"""
import argparse
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
CLASSES = ("move", "fp64", "div/sqrt", "self-max", "lane", "ctl", "vmem", "lds", "smem", "wait", "valu", "salu")
Ins = collections.namedtuple("Ins", "mnem ops target")  # target: label / address of a branch, else None


def classify(mnem, ops):
    if mnem.startswith(("v_mov_", "v_accvgpr_", "v_swap_")):
        return "move"
    if re.match(r"v_(div_scale|div_fmas|div_fixup|rcp|rsq|sqrt)_", mnem):
        return "div/sqrt"
    if mnem.startswith("v_max_"):
        o = [x.strip() for x in ops.split(",")]
        if len(o) == 3 and o[1] == o[2]:
            return "self-max"
    if mnem.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if mnem.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm", "s_call")) or "saveexec" in mnem:
        return "ctl"
    if mnem.startswith("s_") and re.search(r"\bexec(_lo|_hi)?\b", ops):
        return "ctl"
    if mnem.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if mnem.startswith("ds_"):
        return "lds"
    if mnem.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if mnem.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if mnem.startswith("v_"):
        return "fp64" if "_f64" in mnem else "valu"
    return "salu"


def demangled_to_mangled(name):
    """`f<20,2>` -> the prefix `_Z1fILi20ELi2EE` (integer template arguments only); a plain name -> `_Z<len>name`"""
    m = re.fullmatch(r"(\w+)(?:<([-\d, ]+)>)?", name)
    if not m:
        return None
    out = "_Z%d%s" % (len(m.group(1)), m.group(1))
    if m.group(2):
        args = [int(a) for a in m.group(2).split(",")]
        out += "I" + "".join("Li%sE" % (("n%d" % -a) if a < 0 else a) for a in args) + "E"
    return out


def pick(names, want):
    if want in names:
        return want
    pre = demangled_to_mangled(want)
    cand = [n for n in names if pre and n.startswith(pre)] or [n for n in names if want in n]
    if len(cand) != 1:
        sys.exit("%s: %d functions match%s" % (want, len(cand), "".join("\n  " + c for c in cand[:40])))
    return cand[0]


# ------------------------------------------------------------------------------------------------ assembly file
def asm_functions(path):
    names = []
    with open(path, errors="replace") as f:
        for ln in f:
            m = re.match(r"(\w+):\s+; @", ln)
            if m:
                names.append(m.group(1))
    return names


def asm_body(path, sym):
    """(instructions, loop of each instruction (header label or None), loops: header label -> (depth, parent header or None)).  Every
    block carries its innermost loop in the comments behind its label: `in Loop: Header=BBn_m Depth=d`, or for a header its parents
    (`Parent Loop BBn_m Depth=d`) and `This [Inner] Loop Header: Depth=d`."""
    ins, where, loops = [], [], {}
    inside, fresh = False, False  # fresh: between a block's label and its first instruction (the block's comments)
    label, cur, parents = None, None, []
    with open(path, errors="replace") as f:
        for ln in f:
            if not inside:
                inside = ln.startswith(sym + ":")
                continue
            if ln.startswith(".Lfunc_end") or ln.startswith("\t.section") or ln.startswith("\t.end_amdhsa_kernel"):
                break
            code, _, comment = ln.partition(";")
            m = re.match(r"\.L(BB\d+_\d+):", code) or re.match(r"; %bb\.(\d+):", ln)
            if m:
                label, cur, parents, fresh = m.group(1), None, [], True
                comment = comment.partition(";")[2] if ln.startswith("; %bb.") else comment
            if fresh:
                m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
                if m:
                    cur = m.group(1)
                m = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", comment)
                if m:
                    parents.append(m.group(1))
                m = re.search(r"This (Inner )?Loop Header: Depth=(\d+)", comment)
                if m:
                    cur = label
                    loops[label] = (int(m.group(2)), parents[-1] if parents else None)
            code = code.strip()
            if not code or code.startswith(".") or code.endswith(":"):
                continue
            fresh = False
            mnem, _, ops = code.partition(" ")
            ins.append(Ins(mnem, ops.strip(), None))
            where.append(cur)
    return ins, where, loops


# ------------------------------------------------------------------------------------------------ library
def device_code_object(lib, tmpdir):
    data = open(lib, "rb").read()
    at = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if at < 0:
        sys.exit("no uncompressed offload bundle in " + lib)
    (n,) = struct.unpack_from("<Q", data, at + 24)
    p = at + 32
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", data, p)
        p += 24
        triple = data[p:p + tl].decode()
        p += tl
        if "gfx950" in triple:
            out = os.path.join(tmpdir, "device.o")
            with open(out, "wb") as f:
                f.write(data[at + off:at + off + size])
            return out
    sys.exit("no gfx950 code object in " + lib)


def obj_functions(obj):
    r = subprocess.run([OBJDUMP, "-t", obj], capture_output=True, text=True, check=True)
    return [ln.split()[-1] for ln in r.stdout.splitlines() if " F .text" in ln]


def obj_body(obj, sym):
    r = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--disassemble-symbols=" + sym, obj], capture_output=True, text=True, check=True)
    ins, labels = [], {}
    base = None
    for ln in r.stdout.splitlines():
        m = re.match(r"([0-9a-f]+) <%s>:" % re.escape(sym), ln)
        if m:
            base = int(m.group(1), 16)
            continue
        if base is None or not ln.startswith("\t"):
            continue
        code, _, tail = ln.partition("//")
        a = re.match(r"\s*([0-9A-Fa-f]+):", tail)
        if not a:
            continue
        labels[int(a.group(1), 16)] = len(ins)
        mnem, _, ops = code.strip().partition(" ")
        target = None
        if mnem.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(sym), tail)
            target = base + int(t.group(1), 16) if t else (base if "<%s>" % sym in tail else None)
        ins.append(Ins(mnem, ops.strip(), target))
    return (ins,) + backward_branch_loops(ins, labels, sym)


# ------------------------------------------------------------------------------------------------ kernel notes
NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernel_notes(text, substr):
    """the amdhsa.kernels metadata (the tail of an assembly file, or `llvm-readelf --notes` of a code object): one line per kernel whose
    name contains substr - registers, spilled registers, scratch (private segment) and LDS (group segment) bytes"""
    cur = {}
    for ln in text[text.find("amdhsa.kernels"):].splitlines():
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "name" or m.group(1) in NOTE_KEYS:
            cur[m.group(1)] = m.group(2).strip("'")
        if m.group(1) == "wavefront_size":  # (the last key of a kernel's entry)
            if substr in cur.get("name", ""):
                print("%-64s " % cur["name"] + "  ".join("%s %s" % (k.replace("_count", "").replace("_fixed_size", ""), cur.get(k, "-")) for k in NOTE_KEYS))
            cur = {}


# ------------------------------------------------------------------------------------------------ loops, histograms
def backward_branch_loops(ins, labels, sym):
    """a disassembly has no comments: every target of a backward branch counts as a header, its loop reaching to the last branch back to
    it (block placement can make such a branch where the compiler sees no loop: the assembly file is the better input)"""
    end = {}
    for k, i in enumerate(ins):
        if i.target is not None and i.target in labels and labels[i.target] <= k:
            end[i.target] = max(end.get(i.target, -1), k)
    ext = sorted((labels[t], -e, "+0x%x" % (t - min(labels))) for t, e in end.items())  # outer before inner
    where, loops = [None] * len(ins), {}
    for first, neg_last, name in ext:
        parent = where[first]
        if parent is not None and -neg_last > loops[parent][2]:
            continue  # (overlaps its predecessor without nesting in it: not a loop of its own)
        loops[name] = (1 if parent is None else loops[parent][0] + 1, parent, -neg_last)
        for k in range(first, -neg_last + 1):
            where[k] = name
    return where, {n: v[:2] for n, v in loops.items()}


def histogram(ins, idx):
    h = collections.Counter()
    seq = 0
    for k in idx:
        c = classify(ins[k].mnem, ins[k].ops)
        h[c] += 1
        if re.match(r"v_(div_fixup|rsq|sqrt)_", ins[k].mnem):
            seq += 1
    h["sequences"] = seq
    return h


def row(name, h):
    n = sum(h[c] for c in CLASSES)
    return "%-34s %6d " % (name, n) + " ".join("%5d" % h[c] for c in CLASSES) + "  seq %d" % h["sequences"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="libptudes_mi.so, a gfx950 code object, or a --save-temps device .s file")
    ap.add_argument("function", nargs="?", help="mangled name, name<ints>, or a unique substring")
    ap.add_argument("--symbols", metavar="SUBSTR", help="list the function names that contain SUBSTR and exit")
    ap.add_argument("--notes", metavar="SUBSTR", help="print the kernel notes (registers, spills, scratch, LDS) of the kernels whose name contains SUBSTR and exit")
    ap.add_argument("--list", metavar="CLASS", help="also print the instructions of this class ...")
    ap.add_argument("--loop", type=int, metavar="N", help="... of loop number N only (own instructions), as numbered in the table")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        is_asm = a.input.endswith(".s")
        if not is_asm:
            with open(a.input, "rb") as f:
                head = f.read(20)
            obj = a.input if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00" else device_code_object(a.input, tmp)
        names = asm_functions(a.input) if is_asm else obj_functions(obj)
        if a.notes is not None:
            kernel_notes(open(a.input, errors="replace").read() if is_asm else
                         subprocess.run([OBJDUMP.replace("objdump", "readelf"), "--notes", obj], capture_output=True, text=True, check=True).stdout, a.notes)
            return
        if a.symbols is not None:
            print("\n".join(n for n in names if a.symbols in n))
            return
        if not a.function:
            ap.error("function name missing")
        sym = pick(names, a.function)
        ins, where, loops = asm_body(a.input, sym) if is_asm else obj_body(obj, sym)
    if not ins:
        sys.exit(sym + ": no instructions found")
    print("%s  (%s, %d instructions, %d loops)" % (sym, "assembly" if is_asm else "disassembly", len(ins), len(loops)))
    print("%-34s %6s " % ("", "all") + " ".join("%5s" % c[:5] for c in CLASSES))
    print(row("function", histogram(ins, range(len(ins)))))
    own = collections.defaultdict(list)
    for k, w in enumerate(where):
        own[w].append(k)
    order = sorted(loops, key=lambda n: own[n][0] if own[n] else len(ins))  # by the header's place in the text
    kids = collections.defaultdict(list)
    for n in order:
        kids[loops[n][1]].append(n)
    numbered = []

    def show(n):
        def whole(x):
            return own[x] + [k for c in kids[x] for k in whole(c)]
        tag = "%s%d %s d%d" % ("  " * (loops[n][0] - 1), len(numbered), n, loops[n][0])
        numbered.append(n)
        print(row(tag + " all", histogram(ins, whole(n))))
        if kids[n]:
            print(row(tag + " own", histogram(ins, own[n])))
        for c in kids[n]:
            show(c)

    for n in kids[None]:
        show(n)
    if a.list:
        idx = range(len(ins)) if a.loop is None else own[numbered[a.loop]]
        for k in idx:
            if classify(ins[k].mnem, ins[k].ops) == a.list:
                print("%7d  %s %s" % (k, ins[k].mnem, ins[k].ops))


if __name__ == "__main__":
    main()
