#!/usr/bin/env python3
"""Are the kernels of some .hip files instruction-identical between two versions of the tree?  Needs hipcc, no GPU.

    scripts/isa_identity.py PARENT NEW image_io.hip p010.hip [--map old=new ...]

PARENT and NEW are checkouts (their transformerupscaler_amd/csrc and include are used) or csrc directories (include is taken from
../../include of each).  Every file is compiled for gfx950 with the Makefile's language flags and `--cuda-device-only -S`; the output
is split per kernel, comments, labels and directives are stripped and branch targets `.LBB<n>_<k>` are compared as `.LBB_<k>`.
Per kernel one line: `identical`, `DIFFERS`, `parent only` or `new only`, the instructions in NEW (in PARENT for `parent only`) and
the demangled name.  Kernels are paired by that name; `--map old=new` rewrites the substring `old` of a parent name to `new` first,
which pairs renamed kernels: --map 'nv12_to_f32chw_kernel<true>=yuv420_to_f32chw_kernel<Nv12Fmt, true>'.

It compares instruction streams and nothing else: it looks for no particular instruction.  Exit status 0 whatever the verdicts.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile


def dirs(path):
    """(csrc, include) of a checkout or of a csrc directory."""
    inner = os.path.join(path, "transformerupscaler_amd", "csrc")
    if os.path.isdir(inner):
        return inner, os.path.join(path, "include")
    return path, os.path.join(path, "..", "..", "include")


def compile_asm(hipcc, arch, csrc, include, name):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        subprocess.run([hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17", f"-I{include}", "-S", "--cuda-device-only",
                        os.path.join(csrc, name), "-o", out], check=True)
        return open(out).read()


def kernels(asm):
    """{mangled name: [instruction lines]} of the kernels (the symbols that have an .amdhsa_kernel descriptor)."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.split("\n"):
        line = line.split(";")[0].split("//")[0].strip()
        if not line:
            continue
        if line.endswith(":") and " " not in line:
            if line[:-1] in names:
                cur = out.setdefault(line[:-1], [])
            elif line.startswith(".Lfunc_end"):
                cur = None
            continue
        if line.startswith(".") or cur is None:
            continue
        cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(line.split())))
    return out


def short_names(mangled):
    """Demangled names without return type, anonymous namespace and parameter list: kernel<template arguments>."""
    res = {m: m for m in mangled}
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            got = subprocess.run([tool], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
        except (OSError, subprocess.CalledProcessError):
            continue
        res = dict(zip(mangled, got))
        break
    for m, nice in res.items():
        nice = re.sub(r"^void ", "", nice).replace("(anonymous namespace)::", "")
        depth = 0
        for i, ch in enumerate(nice):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                nice = nice[:i]
                break
        res[m] = nice
    return res


def named(asm, maps=()):
    ks = kernels(asm)
    short = short_names(list(ks))
    out = {}
    for m, ins in ks.items():
        name = short[m]
        for old, new in maps:
            name = name.replace(old, new)
        out[name] = ins
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+", help=".hip file names inside csrc")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="pair a renamed kernel: substring of the parent's name = its new text")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    maps = [tuple(m.split("=", 1)) for m in a.map]
    ver = subprocess.run([a.hipcc, "--version"], capture_output=True, text=True).stdout
    hip, clang = re.search(r"HIP version: (\S+)", ver), re.search(r"clang version (\S+)", ver)
    print("command: " + " ".join([os.path.basename(sys.argv[0])] + [f"'{x}'" if re.search(r"[<> ]", x) else x for x in sys.argv[1:]]))
    print(f"compiler: hipcc {hip.group(1) if hip else '?'}, clang {clang.group(1) if clang else '?'}; "
          f"--offload-arch={a.arch} -O3 -std=c++17 -I<include> -S --cuda-device-only <file>")
    print("Per kernel the instruction lines after stripping comments, labels and directives (branch targets .LBB<n>_<k> compared as "
          ".LBB_<k>).\nColumns: verdict, instructions in the new tree (in the parent for `parent only`), kernel.")
    for f in a.files:
        old = named(compile_asm(a.hipcc, a.arch, *dirs(a.parent), f), maps)
        new = named(compile_asm(a.hipcc, a.arch, *dirs(a.new), f))
        print(f"\n== {f}")
        for name in sorted(set(old) | set(new)):
            if name not in new:
                print(f"{'parent only':<12}{len(old[name]):>5}  {name}")
            elif name not in old:
                print(f"{'new only':<12}{len(new[name]):>5}  {name}")
            elif old[name] == new[name]:
                print(f"{'identical':<12}{len(new[name]):>5}  {name}")
            else:
                sm = difflib.SequenceMatcher(None, old[name], new[name], autojunk=False)
                hunks = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
                print(f"{'DIFFERS':<12}{len(new[name]):>5}  {name}  ({len(old[name])} -> {len(new[name])} instructions, {hunks} in differing hunks)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
