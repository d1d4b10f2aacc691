#!/usr/bin/env python3
"""Compare the gfx950 device code of cwfa_amd/csrc between a git revision and the working tree, kernel by kernel.
For refactors that must not change what runs: the set of kernels, each kernel's instruction stream and its descriptor
(.amdhsa_* fields: registers, LDS, scratch) must be equal.  Needs hipcc, no GPU.
    python tools/asm_compare.py [REV] [SOURCE ...]     (REV defaults to main, the sources to build.py's SOURCES)
Exit status 0 when every kernel is identical."""
import os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cwfa_amd import build as b   # noqa: E402


def assemble(tree, src):
    """Device-only assembly of one source in a checkout rooted at `tree`, with the build's flags."""
    csrc, include = os.path.join(tree, "cwfa_amd", "csrc"), os.path.join(tree, "include")
    cmd = [b.HIPCC, *b.FLAGS, *b.EXTRA.get(src, []), "--offload-device-only", "-S", "-o", "-", os.path.join(csrc, src)]
    cmd = [include if a == b.INCLUDE else csrc if a == b.CSRC else a for a in cmd]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr[-3000:]}")
    return r.stdout


def kernels(asm):
    """{kernel symbol: (instruction lines, descriptor lines)}.  Comments and the per-file __hip_cuid_* lines are dropped;
    function-numbered labels (.LBB3_7, .Lfunc_end3) are renumbered by kernel, so that reordering kernels in a file is
    not a difference."""
    lines = [l.split(";")[0].rstrip() for l in asm.splitlines() if "__hip_cuid_" not in l]
    lines = [l for l in lines if l.strip()]
    body, desc, out = {}, {}, {}
    cur = None
    for l in lines:
        m = re.match(r"^([\w$.]+):$", l)
        if m and not l.startswith("."):
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:$", l):
                cur = None
                continue
            body[cur].append(l)
    cur = None
    for l in lines:
        s = l.strip()
        if s.startswith(".amdhsa_kernel "):
            cur = s.split()[1]
            desc[cur] = []
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None:
            desc[cur].append(s)
    for k in desc:
        text = "\n".join(body.get(k, []))
        text = re.sub(r"\.LBB\d+_", ".LBB_", text)
        text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", text)
        out[k] = (text, "\n".join(desc[k]))
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "main"
    sources = sys.argv[2:] or b.SOURCES
    with tempfile.TemporaryDirectory() as base:
        arch = os.path.join(base, "src.tar")
        subprocess.run(["git", "-C", ROOT, "archive", "-o", arch, rev, "cwfa_amd/csrc", "include"], check=True)
        with tarfile.open(arch) as t:
            t.extractall(base)
        jobs = [(tree, s) for s in sources for tree in (base, ROOT)]
        with ThreadPoolExecutor(max_workers=8) as ex:
            asm = list(ex.map(lambda j: assemble(*j), jobs))
    total, bad = 0, 0
    for i, src in enumerate(sources):
        old, new = kernels(asm[2 * i]), kernels(asm[2 * i + 1])
        for k in sorted(set(old) ^ set(new)):
            print(f"{src}: kernel only in {'base' if k in old else 'tree'}: {k}")
            bad += 1
        for k in sorted(set(old) & set(new)):
            total += 1
            for part, what in ((0, "instructions"), (1, "descriptor")):
                if old[k][part] != new[k][part]:
                    print(f"{src}: {what} differ: {k}")
                    bad += 1
        print(f"{src}: {len(new)} kernels", flush=True)
    print(f"{total} kernels compared against {rev}: " + ("all identical" if bad == 0 else f"{bad} differences"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
