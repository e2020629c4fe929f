#!/usr/bin/env python3
"""Did a source change move the kernels' code?  Per kernel symbol: does the gfx950 instruction text differ, and which of the
compiler's resource remarks differ (no GPU).  The check of every "same code, tidier source" change to csrc/.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -c --cuda-device-only -Rpass-analysis=kernel-resource-usage \\
        larynx_amd/csrc/mi355tts.hip -o a.o 2> a.remarks          (once per source state: a and b)
    python tools/isa_diff.py a.o a.remarks b.o b.remarks [--kernels REGEX] > table.md

Only text is compared (llvm-objdump's, without addresses and comments); no instruction is looked for.  Exit status 1 when a
kernel differs."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
REMARKS = ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", r"Occupancy \[waves/SIMD\]")


def tool(name):
    return str(LLVM / name) if (LLVM / name).is_file() else name


def disassembly(obj, tmp):
    """kernel symbol -> its instruction lines"""
    if open(obj, "rb").read(24) == b"__CLANG_OFFLOAD_BUNDLE__":
        elf = str(Path(tmp) / (Path(obj).name + ".elf"))
        subprocess.run([tool("clang-offload-bundler"), "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--input={obj}",
                        f"--output={elf}", "--unbundle"], check=True)
        obj = elf
    text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for ln in text.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(\w+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.strip():
            cur.append(re.sub(r"\s*//.*$", "", ln).strip())  # (comments hold addresses, which move with the kernels before)
    return out


def remarks(path):
    """kernel symbol -> {remark: value}"""
    out = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        vals = {k: re.search(k + r": (\d+)", block) for k in REMARKS}
        out[block.split()[0]] = {k.replace("\\", ""): int(m.group(1)) for k, m in vals.items() if m}
    return out


def demangle(names):
    for filt in (tool("llvm-cxxfilt"), "c++filt"):
        try:
            res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"^void (mi355tts::)?|\(.*$", "", d) for n, d in zip(names, res)}
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("obj_a"), ap.add_argument("remarks_a"), ap.add_argument("obj_b"), ap.add_argument("remarks_b")
    ap.add_argument("--kernels", default="", help="only symbols that match this regular expression")
    ap.add_argument("--all", action="store_true", help="list the identical kernels too")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        da, db = disassembly(args.obj_a, tmp), disassembly(args.obj_b, tmp)
    ra, rb = remarks(args.remarks_a), remarks(args.remarks_b)
    syms = sorted(s for s in set(da) | set(db) if re.search(args.kernels, s))
    names, same = demangle(syms), 0
    print("| kernel | instructions a -> b | text | remarks that differ |\n|---|---|---|---|")
    for s in syms:
        a, b = da.get(s), db.get(s)
        delta = ", ".join(f"{k} {v} -> {rb.get(s, {}).get(k)}" for k, v in ra.get(s, {}).items() if rb.get(s, {}).get(k) != v)
        verdict = "only in a" if b is None else "only in b" if a is None else "identical" if a == b else "differs"
        same += verdict == "identical" and not delta
        if args.all or verdict != "identical" or delta:
            print(f"| `{names[s]}` | {len(a or [])} -> {len(b or [])} | {verdict} | {delta or '-'} |")
    print(f"\n{len(syms)} kernels, {same} identical in text and remarks, {len(syms) - same} not.")
    return 0 if same == len(syms) else 1


if __name__ == "__main__":
    sys.exit(main())
