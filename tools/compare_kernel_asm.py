#!/usr/bin/env python3
"""Device assembly of the kernel translation units in two csrc directories, kernel by kernel (no GPU needed).

    python3 tools/compare_kernel_asm.py <csrc of the parent> <csrc of the tree> [--keep DIR] [--whole FILE.hip ...]

On each side every csrc file whose Makefile rule carries $(KERNEL_SCHED) is compiled (the list is read from that side's
own Makefile, so a kernel that moved to another such file is still compared with itself) by the command that side's
Makefile prints for its object, plus -save-temps=obj; the gfx950 .s files are compared per kernel after dropping
comments, .loc / .file lines and trailing blanks and replacing every .LBB<n>_<m> label and the hash in __hip_cuid_<hash>
(it names the translation unit by its path; the symbol lies outside the kernels) by one token.  Prints `identical` or the number of
differing lines per kernel, and each kernel's VGPRs / AGPRs / scratch / LDS and the waves per SIMD the compiler states
for it.  A kernel is every function label that has an .amdhsa_kernel descriptor, whatever its mangling.  --whole FILE.hip (repeatable): that file's gfx950 .s of both
sides compared WHOLE under the same normalisation (a file in which only host code changed: no line may differ).
Exit status: 0 when every kernel and every whole file is identical, 1 when any differs.
"""
import argparse
import difflib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path


def kernel_sources(csrc: Path) -> list:
    """The .hip files whose object rule in csrc/Makefile carries $(KERNEL_SCHED)."""
    return re.findall(r"^\t.*\$\(KERNEL_SCHED\).* -c -o \$@ (\S+\.hip)$", (csrc / "Makefile").read_text(), re.M)


def build(csrc: Path, source: str, out: Path) -> Path:
    """The .s of one source, by the command the Makefile prints for its object."""
    out.mkdir(parents=True, exist_ok=True)
    stem = source[:-len(".hip")]
    cmd = subprocess.run(["make", "-s", "-n", "-B", "-C", str(csrc), stem + ".o"], check=True, capture_output=True,
                         text=True).stdout.split()
    at = cmd.index("-o")
    cmd[at:at + 2] = ["-save-temps=obj", "-o", str(out / (stem + ".o"))]
    subprocess.run(cmd, check=True, cwd=csrc)
    return out / (stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")


def normalised(raw: str):
    """A line without its comment, or None for a line that does not count."""
    line = raw.split(";", 1)[0].rstrip()
    if not line or re.match(r"\s*\.(loc|file)\s", line):
        return None
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", re.sub(r"\.LBB\d+_\d+", ".LBB", line))


def differing(a, b) -> int:
    return sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))


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
        if normalised(raw) is not None:
            body.append(normalised(raw))
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
    ap.add_argument("--whole", metavar="FILE.hip", action="append", default=[], help="also compare this file's .s whole")
    opt = ap.parse_args()
    keep = opt.keep
    work = Path(keep) if keep else Path(tempfile.mkdtemp(prefix="kernel_asm_"))
    sides = {}
    for side, csrc in (("parent", opt.parent.resolve()), ("tree", opt.tree.resolve())):
        sides[side], sources = {}, kernel_sources(csrc)
        for source in sources:
            found = kernels(build(csrc, source, work / side))
            assert not set(found) & set(sides[side]), "one kernel in two files"
            sides[side].update(found)
        print(f"{side}: {' '.join(sources)}")
    old, new = sides["parent"], sides["tree"]
    pretty = demangle(sorted(set(old) | set(new)))
    unequal = 0
    for n in sorted(set(old) | set(new), key=lambda k: pretty[k]):
        if n not in old or n not in new:
            verdict = "only in the " + ("tree" if n in new else "parent")
        else:
            a, b = old[n][0], new[n][0]
            delta = differing(a, b)
            verdict = "identical" if delta == 0 else f"{delta} differing lines"
        unequal += verdict != "identical"
        r = (new.get(n) or old[n])[1]
        was = old[n][1] if n in old else r
        def show(x):
            return f"VGPRs {x['num_vgpr']:>3}  AGPRs {x['num_agpr']:>2}  scratch {x['private_seg_size']:>3} B  LDS {x['lds']:>5} B  waves/SIMD {x.get('waves', '?')}"
        note = "" if r == was else f"  (parent: {' '.join(show(was).split())})"
        print(f"{pretty[n]:<52} {verdict:<22} {show(r)}{note}")
    print(f"{len(set(old) | set(new))} kernels, {unequal} not identical")
    for source in opt.whole:
        a, b = ([n for n in map(normalised, build(csrc.resolve(), source, work / side).read_text().splitlines()) if n is not None]
                for side, csrc in (("parent", opt.parent), ("tree", opt.tree)))
        delta = differing(a, b)
        unequal += delta != 0
        print(f"{source} whole ({len(b)} lines): " + ("identical" if delta == 0 else f"{delta} differing lines"))
    if not keep:
        shutil.rmtree(work)
    return 1 if unequal else 0


if __name__ == "__main__":
    sys.exit(main())
