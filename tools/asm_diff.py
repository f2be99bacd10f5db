#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel (the evidence a refactor leaves the machine code alone).

    tools/asm_diff.py PARENT_TREE CHANGE_TREE

Compiles every csrc/*.hip of both trees to gfx950 assembly with the Makefile's flags (device side only) and prints, per
file, the kernels that exist on one side only and, per kernel, `identical` or `differs` with the resources of both sides
(VGPRs, SGPRs, LDS bytes, scratch bytes, spilled SGPRs / VGPRs). Kernels are paired by demangled name without the
argument list, so a kernel whose signature changed is compared with its former self. Instruction text is compared with symbol names, local
labels and comments taken out; the compilation-unit id never reaches it.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ["hj_kernels", "hj_build_own", "hj_build_wave", "hj_htm", "hj_pairs", "hj_r_marks", "hj_gather", "hj_keys", "hj_where", "hj_asof", "hj_agg", "hj_sort",
         "hj_prj",      # its translation unit includes hj_prj_pairs.hip and hj_prj_agg.hip: their kernels are listed under it
         "hj_api",
         "hj_api_table", "hj_api_prj", "hj_api_rows", "hj_api_tools"]
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-value --cuda-device-only -S".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_tree(tree, out):
    if os.path.exists(os.path.join(tree, FILES[0] + ".s")):        # a folder of assembly made earlier
        for f in FILES:
            os.symlink(os.path.abspath(os.path.join(tree, f + ".s")), os.path.join(out, f + ".s"))
        return
    src = os.path.join(tree, "htm-hashjoin_amd", "csrc")

    def one(f):
        if not os.path.exists(os.path.join(src, f + ".hip")):       # a file only the other tree has: no kernels on this side
            open(os.path.join(out, f + ".s"), "w").close()
            return
        subprocess.run([HIPCC, *FLAGS, f + ".hip", "-o", os.path.join(out, f + ".s")], cwd=src, check=True,
                       stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(len(FILES)) as ex:
        list(ex.map(one, FILES))


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d).replace("void ", "").replace("hj::", "") for n, d in zip(names, out)}


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


def fmt(r):
    return "%d / %d / %d / %d / %d+%d" % (r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["sspill"], r["vspill"])


def main():
    parent, change = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tc:
        compile_tree(parent, tp)
        compile_tree(change, tc)
        same = differs = 0
        print("| file | kernel | machine code | parent: VGPR / SGPR / LDS / scratch / spills (s+v) | change |")
        print("|---|---|---|---|---|")
        for f in FILES:
            a, b = kernels(os.path.join(tp, f + ".s")), kernels(os.path.join(tc, f + ".s"))
            # paired by demangled name without the argument list: a kernel whose signature changed is still the same kernel
            dm = demangle(sorted(set(a) | set(b)))
            a, b = {dm[k]: v for k, v in a.items()}, {dm[k]: v for k, v in b.items()}
            for k in sorted(set(a) | set(b)):
                if k not in a or k not in b:
                    print("| %s | `%s` | only in %s | %s | %s |" % (f, k, "parent" if k in a else "change",
                                                                   fmt(a[k][1]) if k in a else "", fmt(b[k][1]) if k in b else ""))
                elif a[k][0] == b[k][0] and a[k][1] == b[k][1]:
                    same += 1
                    print("| %s | `%s` | identical | | |" % (f, k))
                else:
                    differs += 1
                    print("| %s | `%s` | differs | %s | %s |" % (f, k, fmt(a[k][1]), fmt(b[k][1])))
        print("\n%d kernels identical, %d differ" % (same, differs))


if __name__ == "__main__":
    main()
