#!/usr/bin/env python3
"""Compare the gfx950 device code of cwfa_amd/csrc between a git revision and the working tree, kernel by kernel.
For refactors that must not change what runs: the set of kernels, each kernel's instruction stream and its descriptor
(.amdhsa_* fields: registers, LDS, scratch) must be equal.  Needs hipcc, no GPU.
    python tools/asm_compare.py [REV] [SOURCE ...] [--rename REGEX=REPLACEMENT ...]
(REV defaults to main, the sources to build.py's SOURCES.)  --rename pairs kernels that a change renamed without changing
their code, such as an added template parameter with a default: the regex is applied to the demangled names at REV (c++filt),
and the kernel it names is compared with the working tree's kernel of the resulting name; each pair is printed.  --allow-new:
kernels only in the working tree (a feature's new instantiations) are listed but are not differences.
Exit status 0 when every kernel is identical."""
import argparse, os, re, subprocess, sys, tarfile, tempfile
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
    function-numbered labels (.LBB3_7, .Lfunc_end3) are renumbered by kernel and the file-numbered anchors of long branches
    (.Lpost_getpc5) lose their number, so that reordering kernels in a file, or adding one, is not a difference."""
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
        text = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", text)     # (long-branch anchors, numbered per file)
        out[k] = (text, "\n".join(desc[k]))
    return out


def demangle(names):
    """{symbol: demangled name} through c++filt."""
    names = list(names)
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def renamed(old, new, rules):
    """{base symbol: tree symbol} for the base-only kernels that a --rename rule maps onto a tree-only kernel."""
    if not rules:
        return {}
    only_old, only_new = set(old) - set(new), set(new) - set(old)
    dm_old, dm_new = demangle(only_old), demangle(only_new)
    by_name = {v: k for k, v in dm_new.items()}
    pairs = {}
    for k in sorted(only_old):
        name = dm_old[k]
        for pat, repl in rules:
            name = re.sub(pat, repl, name)
        if name != dm_old[k] and name in by_name:
            pairs[k] = by_name[name]
    return pairs


def main():
    ap = argparse.ArgumentParser(description="compare device code kernel by kernel between a git revision and the working tree")
    ap.add_argument("rev", nargs="?", default="main")
    ap.add_argument("sources", nargs="*")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT")
    ap.add_argument("--allow-new", action="store_true")
    a = ap.parse_args()
    rev, sources = a.rev, a.sources or b.SOURCES
    rules = [tuple(r.split("=", 1)) for r in a.rename]
    with tempfile.TemporaryDirectory() as base:
        arch = os.path.join(base, "src.tar")
        subprocess.run(["git", "-C", ROOT, "archive", "-o", arch, rev, "cwfa_amd/csrc", "include"], check=True)
        with tarfile.open(arch) as t:
            t.extractall(base)
        jobs = [(tree, s) for s in sources for tree in (base, ROOT)]
        with ThreadPoolExecutor(max_workers=8) as ex:
            asm = list(ex.map(lambda j: assemble(*j), jobs))
    total, bad, npairs, nnew = 0, 0, 0, 0
    for i, src in enumerate(sources):
        old, new = kernels(asm[2 * i]), kernels(asm[2 * i + 1])
        pairs = renamed(old, new, rules)
        for ko, kn in pairs.items():       # compare under the new name; the kernel's own symbol in its text is the name
            print(f"{src}: renamed {ko} -> {kn}")
            old[kn] = tuple(t.replace(ko, kn) for t in old.pop(ko))
        npairs += len(pairs)
        for k in sorted(set(old) ^ set(new)):
            print(f"{src}: kernel only in {'base' if k in old else 'tree'}: {k}")
            if k in new and a.allow_new:
                nnew += 1
            else:
                bad += 1
        for k in sorted(set(old) & set(new)):
            total += 1
            for part, what in ((0, "instructions"), (1, "descriptor")):
                if old[k][part] != new[k][part]:
                    print(f"{src}: {what} differ: {k}")
                    bad += 1
        print(f"{src}: {len(new)} kernels", flush=True)
    extra = (f" ({npairs} of them renamed)" if rules else "") + (f", {nnew} new kernels" if a.allow_new else "")
    print(f"{total} kernels compared against {rev}{extra}: " + ("all identical" if bad == 0 else f"{bad} differences"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
