#!/usr/bin/env python3
"""Instruction mix of the ResBlock MFMA loops, read from the compiler's gfx950 assembly (no GPU).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only larynx_amd/csrc/mi355tts.hip -o dev.s
    python tools/rb_loop_isa.py dev.s > table.md

For every kernel whose name matches --kernels: one row per loop that holds MFMAs (a loop = the lines from a label to the last
backward branch to it; for rb_group_kernel these are the `#pragma unroll 1` chunk loops of rb_tile, one per member), and one row
for the whole kernel (the pair kernels' MFMA phases are straight-line code).  VALU = every v_* instruction except v_mfma*.
profiles/rb_loop_isa.md is this tool's output before and after a change."""
import argparse
import re
import subprocess
import sys

COUNTED = ("v_add_u32", "v_lshl_add_u64", "ds_read2_b32", "ds_read_b32", "global_load_dwordx4")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(text, pattern):
    """name -> (instruction lines with labels, code bytes)"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*\.section", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if not re.search(pattern, name):
            continue
        size = re.search(r"; codeLenInByte = (\d+)", text[m.end():m.end() + 4000])
        out[name] = (body.split("\n"), int(size.group(1)) if size else -1)
    return out


def mix(lines):
    c = dict.fromkeys(("mfma", "valu", "salu") + COUNTED, 0)
    for ln in lines:
        op = ln.split()[0] if ln.split() else ""
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_cbranch", "s_branch", "s_setprio")):
            c["salu"] += 1
        base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)  # encoding suffixes of the VOP forms
        if base in COUNTED:
            c[base] += 1
    return c


def loops(lines):
    """(first line, last line) of every loop with MFMAs that holds no other such loop"""
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    spans = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln) or re.match(r"\s+s_branch\s+(\.LBB\d+_\d+)", ln)
        if m and label_at.get(m.group(1), i) < i:
            spans[label_at[m.group(1)]] = i
    spans = [(a, b) for a, b in spans.items() if any("v_mfma" in ln for ln in lines[a:b])]
    return sorted((a, b) for a, b in spans if not any((c, d) != (a, b) and a <= c and d <= b for c, d in spans))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--kernels", default=r"rb_group_(dil_)?kernel|rb_pair_group_kernel|rbp_dil_group_kernel")
    args = ap.parse_args()
    ks = kernels(open(args.asm).read(), args.kernels)
    names = demangle(sorted(ks))
    head = ["kernel", "span", "MFMA", "VALU", "VALU/MFMA", "SALU"] + list(COUNTED)
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    for name in sorted(ks):
        lines, size = ks[name]
        short = re.sub(r"^void mi355tts::|\(.*$", "", names[name])
        rows = [(f"loop {i}", lines[a:b + 1]) for i, (a, b) in enumerate(loops(lines))] + [(f"whole kernel, {size} B of code", lines)]
        for span, ls in rows:
            c = mix(ls)
            ratio = f"{c['valu'] / c['mfma']:.2f}" if c["mfma"] else "-"
            print("| " + " | ".join([f"`{short}`", span, str(c["mfma"]), str(c["valu"]), ratio, str(c["salu"])] + [str(c[k]) for k in COUNTED]) + " |")
    return 0 if ks else 1


if __name__ == "__main__":
    sys.exit(main())
