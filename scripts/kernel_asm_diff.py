#!/usr/bin/env python3
"""Compare the device code of rap_amd/csrc/*.hip between a git revision and the working tree, kernel by kernel.

    python scripts/kernel_asm_diff.py REV gemm_h16.hip gemm_f32.hip [-DRAP_ABLATION_BUILD ...]

REV's rap_amd/csrc and include are exported into a temporary directory; every listed file is compiled from both trees to
device-only assembly with the flags of rap_amd/_build.py, and for every function symbol the instruction text, the .amdhsa_*
block and the metadata entry are compared.  Lines naming __hip_cuid_ (a hash of the translation unit) are ignored.  Prints one
line per differing kernel and exits 1 if there is any.  Needs hipcc and git, no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
LABEL = re.compile(r"(BB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp)\d+(_?)")      # local labels carry the function's ordinal in the file


def assembly(tree, name, defines):
    r = subprocess.run([HIPCC, *FLAGS, *defines, os.path.join(tree, "rap_amd", "csrc", name), "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed on {tree}/{name}:\n{r.stderr}")
    return r.stdout


def kernels(asm):
    """symbol -> its text: the body with its .amdhsa_kernel block and kernel-info comments, plus its amdgpu_metadata entry"""
    lines = [LABEL.sub(r"\1\2", re.sub(r"(\S)\s+", r"\1 ", l.rstrip())) for l in asm.splitlines() if "__hip_cuid_" not in l]
    out, i = {}, 0
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function$", "\n".join(lines), re.M):
        sym = m.group(1)
        start = next(k for k in range(i, len(lines)) if lines[k].startswith(sym + ":"))
        end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
        # ... and the "; Kernel info:" comment block (register counts, scratch, occupancy) up to the next function's section
        i = end + 1
        while i < len(lines) and lines[i].lstrip().startswith((".size", ".set", ";", ".section .AMDGPU.csdata")):
            i += 1
        out[sym] = lines[start:i]
    entry = None
    for l in lines[lines.index("\t.amdgpu_metadata") if "\t.amdgpu_metadata" in lines else len(lines):]:
        if l.startswith("  - ") or not l.startswith("    "):      # a new kernel entry, or the end of the kernel list
            if entry:
                name = next((e.split(":", 1)[1].strip() for e in entry if e.startswith("    .name:")), None)
                if name:      # (the version list that follows the kernels has items without one)
                    out.setdefault(name, []).extend(entry)
            entry = [l] if l.startswith("  - ") else None
        elif entry:
            entry.append(l)
    return out


def main():
    rev, args = sys.argv[1], sys.argv[2:]
    defines, files = [a for a in args if a.startswith("-D")], [a for a in args if not a.startswith("-D")]
    differing = 0
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "rap_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        with ThreadPoolExecutor(max_workers=8) as ex:
            jobs = [(f, ex.submit(assembly, old, f, defines), ex.submit(assembly, ROOT, f, defines)) for f in files]
            for f, a, b in jobs:
                ka, kb = kernels(a.result()), kernels(b.result())
                for sym in sorted(set(ka) | set(kb)):
                    if ka.get(sym) != kb.get(sym):
                        differing += 1
                        if sym not in ka or sym not in kb:
                            what = "only in " + (rev if sym in ka else "the working tree")
                        else:
                            n = sum(x != y for x, y in zip(ka[sym], kb[sym])) + abs(len(ka[sym]) - len(kb[sym]))
                            first = next(((x, y) for x, y in zip(ka[sym], kb[sym]) if x != y), ("", "(a longer text)"))
                            what = f"{n} of {len(ka[sym])} -> {len(kb[sym])} lines differ, first: {first[0].strip()!r} -> {first[1].strip()!r}"
                        print(f"{f}: {sym}: {what}")
                print(f"{f}: {len(ka)} kernels in {rev}, {len(kb)} in the working tree", file=sys.stderr)
    print(f"{differing} differing kernel(s)" if differing else "no differing kernel")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
