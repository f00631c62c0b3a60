#!/usr/bin/env python3
"""Register, scratch and code-size figures of the venv step / act kernels,
from the code object's metadata (cross-compiled; no device needed).

    tools/venv_items_resources.py [--general] [--heur] [--table] [TREE ...]

For every TREE (default: this one) compiles TREE/dependence_free_rl_amd/csrc/
venv_kernels.hip for the device only, reads each kernel's .vgpr_count,
.sgpr_count and .private_segment_fixed_size from the AMDGPU metadata note and
its code bytes from the symbol table, and prints one JSON line per kernel
(builtin instantiations: venv_step_kernel / venv_act_kernel).  With two trees
it also prints whether the builtin kernels' figures are equal, kernel by
kernel; --general lists the general instantiations (venv_gen_kernels.o)
instead -- the check DESIGN.md 8 records for the general item sets, whose
builtin instantiations are meant to be the parent's code.  --heur reads
venv_heur_kernels.hip (venv_heur_kernel, xh_venv_act_heuristic) instead of
venv_kernels.hip and, beside each kernel, prints the act kernel of the same
shape, mask and episode switches (no distribution record) from
venv_kernels.hip: the heuristic kernel is to need no scratch and no more
VGPRs than it.  --table reads venv_table_kernels.hip (xh_venv_table_*) and
prints venv_act_table_kernel beside the general act kernel of the same shape
and switches, then the other table kernels; none is to need scratch.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = os.environ.get("READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
ARCH = os.environ.get("ARCH", "gfx950")


def kernels(tree, defines=(), unit="venv_kernels.hip"):
    src = os.path.join(tree, "dependence_free_rl_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "venv_kernels.co")
        subprocess.run(
            [HIPCC, "--offload-arch=" + ARCH, "-O3", "-std=c++17",
             "--cuda-device-only", "--no-gpu-bundle-output",
             "-I" + os.path.join(tree, "include"), "-I" + src, *defines, "-c", os.path.join(src, unit),
             "-o", obj], check=True)
        notes = subprocess.run([READELF, "--notes", obj], check=True,
                               capture_output=True, text=True).stdout
        syms = subprocess.run([READELF, "-s", "-W", obj], check=True,
                              capture_output=True, text=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    out = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        def get(key):
            return re.search(r"\.%s:\s*(\S+)" % key, block).group(1)
        name = get("symbol")[:-len(".kd")]
        out[name] = {"vgpr": int(get("vgpr_count")),
                     "sgpr": int(get("sgpr_count")),
                     "scratch": int(get("private_segment_fixed_size")),
                     "lds": int(get("group_segment_fixed_size")),
                     "code_bytes": size.get(name, -1)}
    return out


def demangle(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), check=True,
                         capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, got))


def heur(tree, defines):
    """venv_heur_kernel's figures beside the act kernel's of the same shape."""
    tab = kernels(tree, defines, "venv_heur_kernels.hip")
    act = kernels(tree, defines)
    act = {demangle([n])[n]: v for n, v in act.items()}
    pretty = demangle(sorted(tab))
    bad = []
    for n in sorted(tab, key=pretty.get):
        name = pretty[n]
        m = re.match(r"void xh::venv_heur_kernel<(\d+), (\d+), (\w+), (\w+)"
                     r"(.*)>\(xh::VenvHeurArgs(.*)\)", name)
        if not m:
            continue
        twin = "void xh::venv_act_kernel<%s, %s, false, %s, %s%s>" \
               "(xh::VenvActArgs%s)" % m.groups()
        a = act[twin]
        print(json.dumps({"kernel": name, **tab[n], "act_vgpr": a["vgpr"],
                          "act_code_bytes": a["code_bytes"]}))
        if tab[n]["scratch"] or tab[n]["vgpr"] > a["vgpr"]:
            bad.append(name)
    print(json.dumps({"heur_kernels": len(tab), "scratch_or_more_vgprs": bad}))
    return 1 if bad else 0


def table(tree):
    """The table kernels' figures; the act beside the general act kernel."""
    tab = kernels(tree, (), "venv_table_kernels.hip")
    act = kernels(tree, ("-DXH_VENV_GEN_TU=1",))
    act = {demangle([n])[n]: v for n, v in act.items()}
    pretty = demangle(sorted(tab))
    scratch = []
    for n in sorted(tab, key=pretty.get):
        name, row = pretty[n], dict(tab[n])
        m = re.match(r"void xh::venv_act_table_kernel<(\d+), (\d+), (\w+), "
                     r"(\w+), (\w+)>", name)
        if m:
            a = act["void xh::venv_act_kernel<%s, %s, %s, %s, %s, "
                    "xh::VenvItemTable>(xh::VenvActArgs, xh::VenvItemTable)"
                    % m.groups()]
            row.update(act_vgpr=a["vgpr"], act_code_bytes=a["code_bytes"])
        print(json.dumps({"kernel": name, **row}))
        if tab[n]["scratch"]:
            scratch.append(name)
    print(json.dumps({"table_kernels": len(tab), "scratch": scratch}))
    return 1 if scratch else 0


def main():
    general = "--general" in sys.argv[1:]
    defines = ("-DXH_VENV_GEN_TU=1",) if general else ()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = [t for t in sys.argv[1:]
             if t not in ("--general", "--heur", "--table")] or [here]
    if "--table" in sys.argv[1:]:
        return table(trees[0])
    if "--heur" in sys.argv[1:]:
        return heur(trees[0], defines)
    tables = []
    for t in trees:  # keyed by the demangled name
        tab = kernels(t, defines)
        pretty = demangle(sorted(tab))
        tables.append({pretty[n]: v for n, v in tab.items()})
    for tree, tab in zip(trees, tables):
        for name in sorted(tab):
            print(json.dumps({"tree": tree, "kernel": name, **tab[name]}))
    if len(tables) == 2 and not general:
        a, b = tables
        builtin = [n for n in sorted(a) if re.search(
            r"venv_(step|act)_kernel<[^>]*>\(xh::Venv(Act)?Args\)", n)]
        diff = [n for n in builtin if a[n] != b.get(n)]
        print(json.dumps({"builtin_step_act_kernels": len(builtin),
                          "equal": not diff, "different": diff}))
        return 1 if diff else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
