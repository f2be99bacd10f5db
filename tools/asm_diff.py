#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel (the evidence a refactor leaves the machine code alone).

    tools/asm_diff.py PARENT_TREE CHANGE_TREE

Compiles the .hip files behind the objects of each tree's csrc/Makefile (its OBJS) to gfx950 assembly with the Makefile's
flags (device side only) and prints, per kernel, `identical` or `differs` with the resources of both sides (VGPRs, SGPRs,
LDS bytes, scratch bytes, spilled SGPRs / VGPRs), and the kernels that exist on one side only. Kernels are paired across
the whole library by demangled name without the argument list: a kernel whose signature changed, or that moved to another
file, is compared with its former self and listed under its new file with a note of the old one. A template kernel that
several objects of a tree instantiate is compared copy by copy. Instruction text is compared with symbol names, local
labels and comments taken out; the compilation-unit id never reaches it.

A tree may also be a folder of assembly made earlier (*.s, one per translation unit).
"""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-value --cuda-device-only -S".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_units(src):
    """the translation units of a tree: the objects of its Makefile's OBJS that have a .hip"""
    text = open(os.path.join(src, "Makefile")).read().replace("\\\n", " ")
    objs = re.search(r"^OBJS\s*:?=(.*)$", text, re.M).group(1)
    names = re.findall(r"(\w+)\.o\b", objs)
    return [n for n in names if os.path.exists(os.path.join(src, n + ".hip"))]


def compile_tree(tree, out):
    """-> [(unit, path of its assembly)]"""
    made = sorted(glob.glob(os.path.join(tree, "*.s")))
    if made:                                                        # a folder of assembly made earlier
        return [(os.path.basename(p)[:-2], p) for p in made]
    src = os.path.join(tree, "htm-hashjoin_amd", "csrc")
    units = makefile_units(src)

    def one(f):
        subprocess.run([HIPCC, *FLAGS, f + ".hip", "-o", os.path.join(out, f + ".s")], cwd=src, check=True,
                       stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(min(len(units), os.cpu_count() or 4)) as ex:
        list(ex.map(one, units))
    return [(f, os.path.join(out, f + ".s")) for f in units]


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")).replace("void ", "").replace("hj::", "")
            for n, d in zip(names, out)}


def kernels(path):
    """{symbol: (normalised instruction text, resources)}"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        res[m.group(1)] = {"lds": int(d["group_segment_fixed_size"]), "scratch": int(d["private_segment_fixed_size"])}
    out = {}
    for name, r in res.items():
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        info = text[text.index(".Lfunc_end", text.index("\n" + name + ":")):]
        r["sgpr"] = int(re.search(r"; TotalNumSgprs: (\d+)", info).group(1))
        r["vgpr"] = int(re.search(r"; NumVgprs: (\d+)", info).group(1))
        meta = text[text.rindex("  - .agpr_count", 0, text.index("    .name:           " + name + "\n")):]
        r["sspill"] = int(re.search(r"\.sgpr_spill_count: (\d+)", meta).group(1))
        r["vspill"] = int(re.search(r"\.vgpr_spill_count: (\d+)", meta).group(1))
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].rstrip()
            if not ln:
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\b_Z\w+", "SYM", ln)
            lines.append(ln)
        out[name] = ("\n".join(lines), r)
    return out


def library(units):
    """{kernel name: [(unit, text, resources)]} over a tree's units, in their order"""
    lib = {}
    for unit, path in units:
        ks = kernels(path)
        dm = demangle(sorted(ks))
        for sym in sorted(ks, key=lambda s: dm[s]):
            lib.setdefault(dm[sym], []).append((unit, *ks[sym]))
    return lib


def fmt(r):
    return "%d / %d / %d / %d / %d+%d" % (r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["sspill"], r["vspill"])


def pairs_of(pa, ca):
    """every copy of one kernel with its counterpart: the copy of the same unit if the other side has one, else its first"""
    def partner(x, others):
        return next((o for o in others if o[0] == x[0]), others[0])
    out = [(partner(c, pa), c) for c in ca]
    used = {id(p) for p, _ in out}
    return out + [(p, partner(p, ca)) for p in pa if id(p) not in used]


def compare(parent_units, change_units):
    """-> rows (unit, kernel, verdict, parent resources, change resources), kernels identical, kernels that differ"""
    a, b = library(parent_units), library(change_units)
    rows, same, differs = [], 0, 0
    for k in set(a) | set(b):
        if k not in a or k not in b:
            for unit, _, r in a.get(k) or b[k]:
                rows.append((unit, k, "only in " + ("parent" if k in a else "change"), fmt(r) if k in a else "", fmt(r) if k in b else ""))
            continue
        for p, c in pairs_of(a[k], b[k]):
            note = "" if p[0] == c[0] else " (parent: %s)" % p[0]
            if p[1] == c[1] and p[2] == c[2]:
                same += 1
                rows.append((c[0], k, "identical" + note, "", ""))
            else:
                differs += 1
                rows.append((c[0], k, "differs" + note, fmt(p[2]), fmt(c[2])))
    order = {u: i for i, (u, _) in enumerate(change_units)}
    rows.sort(key=lambda r: (order.get(r[0], len(order)), r[0], r[1], r[2]))
    return rows, same, differs


def main():
    parent, change = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tc:
        rows, same, differs = compare(compile_tree(parent, tp), compile_tree(change, tc))
        print("| file | kernel | machine code | parent: VGPR / SGPR / LDS / scratch / spills (s+v) | change |")
        print("|---|---|---|---|---|")
        for unit, k, verdict, ra, rb in rows:
            print("| %s | `%s` | %s | %s | %s |" % (unit, k, verdict, ra, rb))
        print("\n%d kernels identical, %d differ" % (same, differs))


if __name__ == "__main__":
    main()
