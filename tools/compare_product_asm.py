#!/usr/bin/env python3
"""Compare the gfx950 device code of the product kernels between two source trees.

    python tools/compare_product_asm.py --parent <checkout of the parent commit> [--new <tree>] [--out FILE]

For both trees the product build (the Makefile's CXXFLAGS, no -DSD_CROSSCHECK) of the translation units is compiled with
--cuda-device-only -S: each tree's own SHARED list by default, so a file that was split or renamed needs no mention here.
Kernels are compared by symbol over the union of a tree's files -- one that moved to another product file is still the same
kernel: its instruction stream (comments dropped, local labels renumbered per kernel) and its .amdhsa_ resource block (VGPRs,
SGPRs, LDS, scratch, ...) must be identical.  Kernels may disappear from the product only when they are named in
MOVED_TO_XONLY, and then they must be in one of the new tree's XONLY translation units (the cross-check library).  A kernel
whose argument list this change rewrites has another symbol in the new tree: those named in NEW_ARGUMENTS are paired by their
demangled name without the arguments, and must keep the PINNED fields of the resource block and of the code object's metadata
(registers, scratch, LDS, wavefront and workgroup set-up); their SGPR and instruction counts are reported, not judged.  A
kernel whose body this change rewrites keeps its symbol: for those named in REWRITTEN that differ the LDS (group_segment_fixed_size) must
be equal, the scratch (private_segment_fixed_size) no larger, and the waves per SIMD that the VGPRs allow -- min(8, 512 /
(next_free_vgpr rounded up to 8)) -- no fewer: registers inside one occupancy step cost nothing, scratch and occupancy do.
Their VGPR, SGPR and instruction counts are reported, not judged.  A
kernel that the change adds to the product is expected only when it is named in NEW_KERNELS; any other new symbol is a
mismatch.  Needs hipcc only, no GPU.  Exit status 0: all of that holds.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

MOVED_TO_XONLY = ()            # short names of kernels this change retires from the product into the cross-check library
NEW_ARGUMENTS = ()             # short names of kernels whose argument list this change rewrites
NEW_KERNELS = ()               # short names of kernels this change adds to the product
# short names of kernels whose body this change rewrites
REWRITTEN = ()
PINNED = re.compile(r"next_free_vgpr|accum_offset|vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|"
                    r"wavefront|workgroup|workitem")


def make_var(makefile, name):
    m = re.search(rf"^{name}\s*[:?]?=\s*(.*)$", open(makefile).read(), re.M)
    return m.group(1).strip() if m else ""


def cxxflags(root):
    mk = os.path.join(root, "statdepth_amd", "csrc", "Makefile")
    flags = make_var(mk, "CXXFLAGS")
    for k, v in (("$(ARCH)", "gfx950"), ("$(ROOT)", os.path.abspath(root)), ("$(EXTRA)", "")):
        flags = flags.replace(k, v)
    return flags.split()


def emit(root, fn, outdir, reuse=False):
    out = os.path.join(outdir, fn.replace(".hip", ".s"))
    if reuse and os.path.exists(out):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, *cxxflags(root), "--cuda-device-only", "-S", fn, "-o", out], check=True,
                   cwd=os.path.join(root, "statdepth_amd", "csrc"))
    return out


def kernels(path):
    """{symbol: (instruction lines, resource lines)} of one assembly file"""
    lines = open(path).read().split("\n")
    res, body = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i + 1
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            res[m.group(1)] = [" ".join(x.split()) for x in lines[i + 1:j]]
            i = j
        i += 1
    for sym in res:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        text = []
        for ln in lines[start + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].rstrip()
            if ln.strip():
                text.append(" ".join(ln.split()))
        # local labels carry the function's ordinal in the file (.LBB12_3): renumber in order of first appearance
        names = {}
        def local(m):
            return names.setdefault(m.group(0), ".L%d" % len(names))
        body[sym] = [re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", local, ln) for ln in text]
    # the code object's metadata of the kernel (.vgpr_count, .agpr_count, .sgpr_count, .max_flat_workgroup_size, ...)
    meta = {}
    for entry in re.split(r"\n  - ", open(path).read().split("amdhsa.kernels:")[-1]):
        nm = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
        if nm and nm.group(1) in res:
            meta[nm.group(1)] = [f".meta{k} {v}" for k, v in re.findall(r"^\s*(\.(?:[asv]gpr_count|max_flat_workgroup_size|"
                                                                       r"wavefront_size)):\s+(\S+)", entry, re.M)]
    return {s: (body[s], res[s] + meta.get(s, [])) for s in res}


def short_name(name):
    return name.split("::")[-1].split("<")[0]


def demangle(sym):
    r = subprocess.run(["c++filt", sym], capture_output=True, text=True)
    name = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else sym
    return re.sub(r"\(.*", "", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="root of a checkout of the parent commit")
    ap.add_argument("--new", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--workdir", default=None, help="keep the assembly files here (default: a temporary directory)")
    ap.add_argument("--reuse", action="store_true", help="do not recompile assembly files that --workdir already holds")
    a = ap.parse_args()
    report = []
    ok = True
    with tempfile.TemporaryDirectory() as tmpdir:
        tmp = a.workdir or tmpdir
        def unit_list(root, var):
            return make_var(os.path.join(root, "statdepth_amd", "csrc", "Makefile"), var).split()
        units = {"parent": unit_list(a.parent, "SHARED"), "new": unit_list(a.new, "SHARED"), "xonly": unit_list(a.new, "XONLY")}
        roots = {"parent": a.parent, "new": a.new, "xonly": a.new}
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            for tag, fns in units.items():
                os.makedirs(os.path.join(tmp, tag), exist_ok=True)
                for fn in fns:
                    jobs[(tag, fn)] = ex.submit(emit, roots[tag], fn, os.path.join(tmp, tag), a.reuse)
        where, asm = {}, {}                              # per tree: symbol -> file, symbol -> (instructions, resources)
        for (tag, fn), f in jobs.items():
            for sym, k in kernels(f.result()).items():
                assert sym not in asm.setdefault(tag, {}), f"{sym} is defined in two {tag} units"
                asm[tag][sym] = k
                where.setdefault(tag, {})[sym] = fn
        old, new = asm.get("parent", {}), asm.get("new", {})
        xonly_names = {demangle(s) for s in asm.get("xonly", {})}
        same = moved = rewritten = 0
        renamed = {demangle(s): s for s in set(new) - set(old) if short_name(demangle(s)) in NEW_ARGUMENTS}
        for sym in sorted(old):
            name = demangle(sym)
            if sym not in new and name in renamed:
                nsym = renamed.pop(name)
                pin = lambda res: sorted(ln for ln in res if PINNED.search(ln))
                was, now = pin(old[sym][1]), pin(new[nsym][1])
                sg = lambda res: next((ln.split()[-1] for ln in res if ln.startswith(".meta.sgpr_count")), "?")
                report.append(f"{where['new'][nsym]}: {name}: new arguments, pinned fields {'same' if was == now else 'DIFFER'}; "
                              f"SGPRs {sg(old[sym][1])} -> {sg(new[nsym][1])}, instructions {len(old[sym][0])} -> "
                              f"{len(new[nsym][0])}")
                if was != now:
                    ok = False
                    report.extend(f"    {x}  ->  {y}" for x, y in zip(was, now) if x != y)
                continue
            if sym not in new:
                short = short_name(name)
                allowed = short in MOVED_TO_XONLY and name in xonly_names
                ok &= allowed
                report.append(f"{where['parent'][sym]}: {name}: left the product, " +
                              ("present in an XONLY unit: allowed" if allowed else "NOT ALLOWED"))
                continue
            if short_name(name) in REWRITTEN and old[sym] != new[sym]:      # (an instantiation that did not change counts as identical)
                def num(res, field):
                    return next(int(ln.split()[-1]) for ln in res if ln.split()[0] == field)
                def waves(res):                          # per SIMD, as the registers allow: VGPRs are allocated in blocks of 8 of 512
                    return min(8, 512 // (-(-num(res, ".amdhsa_next_free_vgpr") // 8) * 8))
                was, now = old[sym][1], new[sym][1]
                lds = [num(r, ".amdhsa_group_segment_fixed_size") for r in (was, now)]
                scratch = [num(r, ".amdhsa_private_segment_fixed_size") for r in (was, now)]
                occ = [waves(r) for r in (was, now)]
                vg = [num(r, ".amdhsa_next_free_vgpr") for r in (was, now)]
                good = lds[0] == lds[1] and scratch[1] <= scratch[0] and occ[1] >= occ[0]
                sg = lambda res: next((ln.split()[-1] for ln in res if ln.startswith(".meta.sgpr_count")), "?")
                rewritten += 1
                report.append(f"{where['new'][sym]}: {name}: rewritten, {'ok' if good else 'WORSE'}; LDS {lds[0]} -> {lds[1]}, "
                              f"scratch {scratch[0]} -> {scratch[1]}, waves per SIMD {occ[0]} -> {occ[1]}; VGPRs {vg[0]} -> "
                              f"{vg[1]}, SGPRs {sg(was)} -> {sg(now)}, instructions {len(old[sym][0])} -> {len(new[sym][0])}")
                ok &= good
                continue
            code = old[sym][0] == new[sym][0]
            resources = old[sym][1] == new[sym][1]
            if code and resources:
                same += 1
                if where["parent"][sym] != where["new"][sym]:
                    moved += 1
                    report.append(f"{name}: identical, moved {where['parent'][sym]} -> {where['new'][sym]}")
            else:
                ok = False
                report.append(f"{where['new'][sym]}: {name}: DIFFERS (instructions {'same' if code else 'differ'}, "
                              f"resource block {'same' if resources else 'differs'})")
        for sym in sorted(s for s in set(new) - set(old) if short_name(demangle(s)) not in NEW_ARGUMENTS
                          or demangle(s) in renamed):
            expected = short_name(demangle(sym)) in NEW_KERNELS
            ok &= expected
            report.append(f"{where['new'][sym]}: {demangle(sym)}: NEW in the product" + (", expected" if expected else ""))
        insts = sum(len(old[s][0]) for s in old if s in new)
        report.append(f"{len(units['parent'])} product files in the parent, {len(units['new'])} in the new tree")
        report.append(f"{len(old)} kernels in the parent, {len(new)} in the new tree, {same} identical (instruction stream, "
                      f"{insts} lines, and .amdhsa_ block), {moved} of them in another file, {rewritten} rewritten")
    report.append("RESULT: " + ("product kernels unchanged" if ok else "MISMATCH"))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
