#!/usr/bin/env python3
"""Device assembly of vgicp_kernels.hip in two csrc directories, kernel by kernel (no GPU needed).

    python3 tools/compare_kernel_asm.py <csrc of the parent> <csrc of the tree> [--keep DIR]

Each directory's vgicp_kernels.hip is compiled with its own Makefile's HIPCC, HIPFLAGS and KERNEL_SCHED plus
-save-temps=obj; the two gfx950 .s files are compared per kernel after dropping comments, .loc / .file lines and
trailing blanks and replacing every .LBB<n>_<m> label by one token (the __hip_cuid_* symbol lies outside the kernels).
Prints `identical` or the number of differing lines per kernel, and each kernel's VGPRs / AGPRs / scratch / LDS and
the waves per SIMD the compiler states for it.  A kernel is every function label that has an .amdhsa_kernel
descriptor, whatever its mangling.  Exit status: 0 when every kernel is identical, 1 when any differs.
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ASM = "vgicp_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"


def build(csrc: Path, out: Path) -> Path:
    out.mkdir(parents=True, exist_ok=True)
    flags = subprocess.run(
        ["make", "-s", "-C", str(csrc), "--eval", "print-flags: ; @echo $(HIPCC) $(HIPFLAGS) $(KERNEL_SCHED)", "print-flags"],
        check=True, capture_output=True, text=True).stdout.split()
    subprocess.run(flags + ["-save-temps=obj", "-c", "-o", str(out / "k.o"), "vgicp_kernels.hip"], check=True, cwd=csrc)
    return out / ASM


def kernels(path: Path) -> dict:
    """name -> (normalised body lines, resource line)"""
    found, name, body = {}, None, []
    res, last = {}, None
    for raw in path.read_text().splitlines():
        m = re.match(r"\s*\.set (\S+)\.(num_vgpr|num_agpr|private_seg_size), (\d+)", raw)
        if m:
            res.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
        m = re.match(r"\s*\.amdhsa_group_segment_fixed_size (\d+)", raw)
        if m and last:
            res.setdefault(last, {})["lds"] = m.group(1)
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", raw)
        if m:
            last = m.group(1)
        m = re.match(r"; Occupancy: (\d+)", raw)
        if m and found:
            res.setdefault(list(found)[-1], {})["waves"] = m.group(1)
        line = raw.split(";", 1)[0].rstrip()
        if name is None:
            m = re.match(r"([A-Za-z_][\w$.]*):$", line)
            if m:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            found[name], name = body, None
            continue
        if not line or re.match(r"\s*\.(loc|file)\s", line):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", line))
    return {k: (v, res.get(k, {})) for k, v in found.items() if "lds" in res.get(k, {})}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(anonymous namespace\)::|vgicp::", "", d).split("(")[0] for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", type=Path, help="csrc directory of the parent tree")
    ap.add_argument("tree", type=Path, help="csrc directory of the tree")
    ap.add_argument("--keep", metavar="DIR", help="keep the compiler's intermediate files there")
    opt = ap.parse_args()
    keep = opt.keep
    work = Path(keep) if keep else Path(tempfile.mkdtemp(prefix="kernel_asm_"))
    old = kernels(build(opt.parent.resolve(), work / "parent"))
    new = kernels(build(opt.tree.resolve(), work / "tree"))
    pretty = demangle(sorted(set(old) | set(new)))
    differing = 0
    for n in sorted(set(old) | set(new), key=lambda k: pretty[k]):
        if n not in old or n not in new:
            verdict = "only in the " + ("tree" if n in new else "parent")
        else:
            a, b = old[n][0], new[n][0]
            delta = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            verdict = "identical" if delta == 0 else f"{delta} differing lines"
        differing += verdict != "identical"
        r = (new.get(n) or old[n])[1]
        was = old[n][1] if n in old else r
        def show(x):
            return f"VGPRs {x['num_vgpr']:>3}  AGPRs {x['num_agpr']:>2}  scratch {x['private_seg_size']:>3} B  LDS {x['lds']:>5} B  waves/SIMD {x.get('waves', '?')}"
        note = "" if r == was else f"  (parent: {' '.join(show(was).split())})"
        print(f"{pretty[n]:<52} {verdict:<22} {show(r)}{note}")
    print(f"{len(set(old) | set(new))} kernels, {differing} not identical")
    if not keep:
        shutil.rmtree(work)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
