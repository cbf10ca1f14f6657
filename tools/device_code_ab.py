#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?  No GPU needed.

    python tools/device_code_ab.py PARENT_TREE CHANGE_TREE [--jobs N] > table.md

Every .hip file of each tree's replay_cql_amd/build.py SOURCES is compiled with that tree's flags for the file plus
`--cuda-device-only -S`.  The assembly is cut per function symbol (code, kernel descriptor, resource comments, metadata
entry); `.file`, `.ident`, the `__hip_cuid_<hash>` symbol (a hash of the source text), the per-file numbers in local
labels and the comment column are dropped.  A file both trees have is compared with itself; the kernels of a new file are
looked up by symbol wherever the parent had them, so code that moved is compared with where it came from.  Prints a
Markdown table per CHANGE file and exits 1 on any difference, on a missing and on a new symbol."""
from __future__ import annotations

import re
import runpy
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path


def recipe(tree: Path):
    ns = runpy.run_path(str(tree / "replay_cql_amd" / "build.py"), run_name="recipe")
    return ns["SOURCES"], ns["EXTRA"], ns["ARCH"]


def assembly(tree: Path, src: str, extra: list, arch: str, tmp: Path) -> str:
    tmp.mkdir(parents=True, exist_ok=True)
    out = tmp / (src + ".s")
    subprocess.run(["hipcc", f"--offload-arch={arch}", "-O3", "-fPIC", "-std=c++17", *extra, "--cuda-device-only", "-S",
                    str(tree / "replay_cql_amd" / "csrc" / src), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


LABEL = re.compile(r"(\.L(?:BB|func_begin|func_end|tmp|JTI)|\bBB)\d+")   # also "Header=BB6_28" in loop comments


def cut(asm: str) -> dict:
    """symbol -> (normalised text, code bytes, is_kernel)"""
    lines = [ln for ln in asm.splitlines()
             if not ln.lstrip().startswith((".file", ".ident")) and "__hip_cuid_" not in ln]
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) if (m := re.match(r"\s*\.type\s+(\S+),@function", ln))]
    meta_at = next((i for i, ln in enumerate(lines) if ".amdgpu_metadata" in ln), len(lines))
    meta, cur = {}, None
    for ln in lines[meta_at:]:
        if ln.startswith("  - "):
            cur = []
        elif not ln.startswith(" "):
            cur = None                                   # behind the last kernel's entry
        if cur is not None:
            cur.append(ln)
            if (m := re.match(r"\s+\.symbol:\s+(\S+)\.kd", ln)):
                meta[m.group(1)] = cur
    funcs = {}
    for n, (i, sym) in enumerate(starts):
        j = starts[n + 1][0] if n + 1 < len(starts) else meta_at
        body = lines[i:j]
        # up to .size and the resource comments behind it: not the next symbol's preamble, not the file's trailer
        end = next(k for k, ln in enumerate(body) if re.match(r"\s*\.size\s+" + re.escape(sym) + ",", ln)) + 1
        while end < len(body) and (not body[end].strip() or body[end].lstrip().startswith((";", ".set " + sym + ".")) or
                                   ".AMDGPU.csdata" in body[end]):
            end += 1
        body = body[:end]
        text = LABEL.sub(lambda m: m.group(1), "\n".join(body + meta.get(sym, [])))
        text = re.sub(r"[ \t]+;", " ;", text)            # comments are aligned to a column: a shorter label moves them
        seen = {}                                        # long-branch labels are counted per file: recount per function
        text = re.sub(r"\.Lpost_getpc\d+", lambda m: f".Lpost_getpc#{seen.setdefault(m.group(0), len(seen))}", text)
        size = next((int(m.group(1)) for ln in body if (m := re.search(r"codeLenInByte = (\d+)", ln))), 0)
        funcs[sym] = (text, size, any(".amdhsa_kernel" in ln for ln in body))
    return funcs


def library(tree: Path, jobs: int, tmp: Path) -> dict:
    sources, extra, arch = recipe(tree)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        texts = list(ex.map(lambda s: assembly(tree, s, extra.get(s, []), arch, tmp), sources))
    return {s: cut(t) for s, t in zip(sources, texts)}


def main() -> int:
    parent, change = Path(sys.argv[1]).resolve(), Path(sys.argv[2]).resolve()
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 8
    with tempfile.TemporaryDirectory() as t:
        a, b = library(parent, jobs, Path(t) / "a"), library(change, jobs, Path(t) / "b")
    old = {sym: (src, f) for src, fs in a.items() for sym, f in fs.items()}
    new = {sym: (src, f) for src, fs in b.items() for sym, f in fs.items()}
    bad = 0
    print("| file | from | functions (kernels) | code bytes | identical |")
    print("|---|---|---|---|---|")
    for src, fs in b.items():
        # a file the parent has is compared with itself (library templates are instantiated in several files, each with
        # its own copy); a new file's kernels are looked up wherever the parent had them
        was = {s: (src, a[src][s]) for s in fs if s in a.get(src, {})} if src in a else {s: old[s] for s in fs if s in old}
        origin = sorted({w[0] for w in was.values()})
        differ = sorted(s for s, f in fs.items() if s not in was or was[s][1][0] != f[0])
        bad += len(differ)
        print(f"| {src} | {', '.join(origin) if origin != [src] else 'same'} | {len(fs)} ({sum(f[2] for f in fs.values())}) | "
              f"{sum(f[1] for f in fs.values())} | {'yes' if not differ else f'NO: {len(differ)}, first {differ[0][:80]}'} |")
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    n_old = sum(f[1][2] for f in old.values())
    print(f"\nparent: {len(old)} function symbols ({n_old} kernels) in {len(a)} files; change: {len(new)} "
          f"({sum(f[1][2] for f in new.values())} kernels) in {len(b)} files; missing: {len(missing)} {[s[:80] for s in missing[:5]]}; new: {len(added)} {[s[:80] for s in added[:5]]}")
    return 1 if bad or missing or added else 0


if __name__ == "__main__":
    sys.exit(main())
