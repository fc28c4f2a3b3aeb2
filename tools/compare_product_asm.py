#!/usr/bin/env python3
"""Compare the gfx950 device code of the product rank kernels between two source trees.

    python tools/compare_product_asm.py --parent <checkout of the parent commit> [--new <tree>] [--out FILE]

For both trees the product build (the Makefile's CXXFLAGS, no -DSD_CROSSCHECK) of FILES is compiled with
--cuda-device-only -S.  Per kernel symbol the instruction stream (comments dropped, local labels renumbered per kernel) and
the .amdhsa_ resource block (VGPRs, SGPRs, LDS, scratch, ...) must be identical.  Kernels may disappear from the product
only when they are named in ALLOWED_TO_LEAVE, and then they must be in one of the new tree's XONLY translation units (the
cross-check library).  Needs hipcc only, no GPU.  Exit status 0: all of that holds.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FILES = ("mbd_rank_ab.hip", "mbd_rank_big.hip", "mbd_rank_bucket.hip", "band_enum.hip")
ALLOWED_TO_LEAVE = ("chunk_sort_kernel", "chunk_search_kernel", "bucket_search_kernel")


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
    return {s: (body[s], res[s]) for s in res}


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
        xonly = make_var(os.path.join(a.new, "statdepth_amd", "csrc", "Makefile"), "XONLY").split()
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
            for tag, root, fns in (("parent", a.parent, FILES), ("new", a.new, FILES), ("xonly", a.new, xonly)):
                os.makedirs(os.path.join(tmp, tag), exist_ok=True)
                for fn in fns:
                    jobs[(tag, fn)] = ex.submit(emit, root, fn, os.path.join(tmp, tag), a.reuse)
        asm = {k: kernels(f.result()) for k, f in jobs.items()}
        xonly_names = {demangle(s) for (tag, _), ks in asm.items() if tag == "xonly" for s in ks}
        for fn in FILES:
            old, new = asm[("parent", fn)], asm[("new", fn)]
            same = 0
            for sym in sorted(old):
                name = demangle(sym)
                if sym not in new:
                    short = name.split("::")[-1].split("<")[0]
                    allowed = short in ALLOWED_TO_LEAVE and name in xonly_names
                    ok &= allowed
                    report.append(f"{fn}: {name}: left the product, " +
                                  ("present in an XONLY unit: allowed" if allowed else "NOT ALLOWED"))
                    continue
                code = old[sym][0] == new[sym][0]
                resources = old[sym][1] == new[sym][1]
                if code and resources:
                    same += 1
                else:
                    ok = False
                    report.append(f"{fn}: {name}: DIFFERS (instructions {'same' if code else 'differ'}, "
                                  f"resource block {'same' if resources else 'differs'})")
            for sym in sorted(set(new) - set(old)):
                ok = False
                report.append(f"{fn}: {demangle(sym)}: NEW in the product")
            insts = sum(len(old[s][0]) for s in old if s in new)
            report.append(f"{fn}: {len(old)} kernels in the parent, {len(new)} in the new tree, {same} identical "
                          f"(instruction stream, {insts} lines, and .amdhsa_ block)")
    report.append("RESULT: " + ("product kernels unchanged" if ok else "MISMATCH"))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
