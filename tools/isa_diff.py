#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel (the check of a kernel refactor that must not
change code: run it on a CPU-only machine, hipcc cross-compiles).

    tools/isa_diff.py PARENT/dl-unet_amd/csrc NEW/dl-unet_amd/csrc [FILE.hip ...]     (default: every *.hip of PARENT)

Each file of both trees is compiled with  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S;  comments,
.file / .ident / .loc / .cfi lines and the __hip_cuid_* symbol are dropped, a kernel's own symbol and the function
numbers in local labels are normalised, and per kernel the instruction stream, the .amdhsa_* lines and the metadata
resource lines (VGPRs, SGPRs, LDS, scratch, kernarg size) are compared.  Kernels are paired by mangled name, per file; a kernel
that has left its file is looked up by that name in the other *.hip of NEW (it moved: same check, no --allow); kernels left
over on both sides (a template parameter was removed: the symbol changes) are paired when their normalised code is equal.
Exit status 0 iff every kernel of the parent has an identical partner or matches --allow REGEX (kernels that are meant to
change, their resource lines are printed, or to go: an instantiation nothing launches); -v prints a unified diff of those
that differ.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ["igemm.hip", "igemmx.hip", "igemmb.hip", "wino.hip", "wgrad.hip", "wgradw.hip"]     # if PARENT lists no *.hip
META_KEYS = (".agpr_count", ".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".uses_dynamic_stack")
DROP = re.compile(r"^\s*(;|\.file\b|\.ident\b|\.loc\b|\.cfi_|\.p2align\b|\.section\b|\.text\b|\.protected\b|\.globl\b|\.weak\b|\.size\b|\.set\b)")


def compile_s(hipcc, src, out):
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, stderr=subprocess.DEVNULL, cwd=os.path.dirname(src))
    with open(out) as f:
        return f.read().splitlines()


def kernels(lines):
    """{mangled name: normalised lines} of one assembly file"""
    out, name, body = {}, None, []
    meta, in_meta, entry = {}, False, []

    def close_entry():
        nm = [l.split(":", 1)[1].strip() for l in entry if l.strip().startswith(".name:")]
        if nm:
            meta[nm[0]] = [l.strip() for l in entry if l.strip().split(":")[0].lstrip("- ") in META_KEYS]

    for l in lines:
        if l.startswith("\t.amdgpu_metadata"):
            in_meta = True
            continue
        if in_meta:
            if l.startswith("  - ") or l.startswith("\t.end_amdgpu_metadata") or l.startswith("amdhsa."):
                close_entry()
                entry = []
            entry.append(l)
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", l)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if l.strip() == ".end_amdhsa_kernel":
            out[name] = body
            name = None
            continue
        if DROP.match(l) or not l.strip() or "__hip_cuid_" in l:
            continue
        l = re.sub(r"\s+;.*$", "", l).replace(name, "@KERNEL")
        l = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", l)
        body.append(l.rstrip())
    for k in out:
        out[k] = out[k] + ["meta " + x for x in sorted(meta.get(k, []))]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-v", action="store_true", help="print the differing lines")
    ap.add_argument("--allow", default=None, metavar="REGEX", help="demangled kernel names that may differ")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    a.files = a.files or sorted(f for f in os.listdir(a.parent) if f.endswith(".hip")) or FILES
    demangle = lambda s: subprocess.run(["c++filt", s], capture_output=True, text=True).stdout.strip() or s
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as ex:
        new_files = sorted(set(a.files) | {f for f in os.listdir(a.new) if f.endswith(".hip")})
        jobs = {(side, f): ex.submit(compile_s, a.hipcc, os.path.join(os.path.abspath(d), f), os.path.join(tmp, side + "_" + f + ".s"))
                for side, d, fs in (("a", a.parent, a.files), ("b", a.new, new_files)) for f in fs}
        new = {f: kernels(jobs[("b", f)].result()) for f in new_files}
        for f in a.files:
            ka, kb = kernels(jobs[("a", f)].result()), dict(new[f])
            for n in [n for n in ka if n not in kb]:      # a kernel that left this file: its new home, by mangled name
                home = next((g for g in new_files if n in new[g]), None)
                if home:
                    kb[n] = new[home][n]
                    print("%s: %s is now in %s" % (f, demangle(n), home))
            pairs = [(n, n) for n in ka if n in kb]
            left_a, left_b = [n for n in ka if n not in kb], [n for n in kb if n not in ka]
            for n in list(left_a):                       # renamed symbols: pair by equal code, else in order of appearance
                twin = next((m for m in left_b if kb[m] == ka[n]), None)
                if twin:
                    pairs.append((n, twin)); left_a.remove(n); left_b.remove(twin)
            pairs += list(zip(left_a, left_b))
            same = 0
            for na, nb in pairs:
                if ka[na] == kb[nb]:
                    same += 1
                    continue
                allowed = bool(a.allow and re.search(a.allow, demangle(na)))
                bad += 0 if allowed else 1
                d = [x for x in difflib.unified_diff(ka[na], kb[nb], lineterm="", n=2)]
                nd = sum(1 for x in d if x[:1] in "+-" and x[:3] not in ("+++", "---"))
                res = "; ".join(x[5:] for x in kb[nb] if x.startswith("meta ") and x not in ka[na])
                print("%s: %s %s  (%d -> %d instructions/lines, %d differing%s)" %
                      (f, "changed (allowed)" if allowed else "DIFFERENT", demangle(na), len(ka[na]), len(kb[nb]), nd, "; new " + res if res else ""))
                if a.v:
                    print("\n".join(d))
            for n in left_a[len(left_b):]:
                allowed = bool(a.allow and re.search(a.allow, demangle(n)))
                bad += 0 if allowed else 1
                print("%s: only in parent%s: %s" % (f, " (allowed)" if allowed else "", demangle(n)))
            for n in left_b[len(left_a):]:
                print("%s: only in new: %s" % (f, demangle(n)))
            print("%s: %d of %d kernels identical" % (f, same, len(ka)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
