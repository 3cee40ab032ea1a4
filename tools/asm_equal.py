#!/usr/bin/env python3
"""Compare the kernels of two AMDGPU assembly files (hipcc --cuda-device-only -S) by demangled name.

    tools/asm_equal.py [--scalar-ok] [--sub PATTERN REPL ...] OLD.s NEW.s
                                                  (several translation units: concatenate their .s files)

Per kernel: IDENTICAL when the instruction stream (comments, labels and symbol names dropped) and the
resource lines (.amdhsa_* descriptor, occupancy, register / scratch / LDS counts) are equal; SCALAR-ONLY
when the instruction count and the resource lines are equal and so is the subsequence of instructions that
do not start with `s_` (every vector, LDS, memory and MFMA instruction is the same text in the same order:
only scalar instructions were reordered or renumbered); otherwise the number of differing instruction
lines and the resource lines that moved.  Exit status 1 if any kernel is not identical or exists on one
side only; with --scalar-ok the SCALAR-ONLY kernels, counted separately, do not set it.
"""
import difflib
import re
import shutil
import subprocess
import sys

CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
RES_COMMENT = re.compile(r";\s*(Occupancy|NumVgprs|NumAgprs|TotalNumVgprs|TotalNumSgprs|ScratchSize|LDSByteSize)\b.*")


def parse(path):
    """{mangled kernel name: (instruction lines, resource lines)}"""
    kernels, body, res = {}, {}, {}
    cur = None       # function being read
    last = None      # function just ended (its resource comments follow)
    desc = None      # kernel descriptor being read
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.strip()
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                cur, last = m.group(1), None
                body[cur], res[cur] = [], []
                continue
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:  # (the descriptor sits inside the function's text, before its end label)
                desc = m.group(1)
                continue
            if desc is not None:
                if line.startswith(".end_amdhsa_kernel"):
                    kernels[desc] = None
                    desc = None
                elif line.startswith(".amdhsa_"):
                    res.setdefault(desc, []).append(line.split(";", 1)[0].strip())
                continue
            if cur is not None:
                if re.match(r"\.Lfunc_end\d+:", line):
                    cur, last = None, cur
                    continue
                code = line.split(";", 1)[0].strip()
                if not code or code.startswith(".") or re.match(r"^[\w.$]+:$", code):  # directives, labels
                    continue
                code = re.sub(r"\.LBB\d+_", ".LBB_", code)
                code = re.sub(r"\b_Z\w+", "SYM", code)
                body[cur].append(code)
                continue
            if last is not None and RES_COMMENT.match(line):
                res[last].append(line)
    return {k: (body.get(k, []), res.get(k, [])) for k in kernels}


def demangle(names):
    if CXXFILT is None:  # (no demangler on the path: the mangled names still pair the kernels)
        return {n: n for n in names}
    out = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def verdict(old, new):
    """IDENTICAL, SCALAR-ONLY or DIFFERS for two (instruction lines, resource lines) pairs"""
    (bo, ro), (bn, rn) = old, new
    if ro != rn or len(bo) != len(bn):
        return "DIFFERS"
    if bo == bn:
        return "IDENTICAL"
    vector = lambda body: [i for i in body if not i.startswith("s_")]
    return "SCALAR-ONLY" if vector(bo) == vector(bn) else "DIFFERS"


def main():
    # --sub PATTERN REPL (repeatable, before the files): a regex substitution on the demangled names of both
    # sides, for a kernel whose name changed but whose code should not have (a new defaulted template flag)
    subs = []
    scalar_ok = False
    while len(sys.argv) > 1 and sys.argv[1] in ("--sub", "--scalar-ok"):
        if sys.argv[1] == "--scalar-ok":
            scalar_ok = True
            del sys.argv[1]
            continue
        if len(sys.argv) <= 4:
            sys.exit(__doc__)
        subs.append((re.compile(sys.argv[2]), sys.argv[3]))
        del sys.argv[1:4]
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    dm = demangle(sorted(set(old) | set(new)))
    for pat, repl in subs:
        dm = {k: pat.sub(repl, v) for k, v in dm.items()}
    old = {dm[k]: v for k, v in old.items()}
    new = {dm[k]: v for k, v in new.items()}
    bad = scalar = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{'ONLY IN NEW' if name in new else 'ONLY IN OLD'}  {name}")
            bad += 1
            continue
        (bo, ro), (bn, rn) = old[name], new[name]
        v = verdict(old[name], new[name])
        if v == "IDENTICAL":
            print(f"IDENTICAL  {name}  ({len(bo)} instructions)")
            continue
        moved = sum(1 for d in difflib.unified_diff(bo, bn, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
        if v == "SCALAR-ONLY":
            scalar += 1
            print(f"SCALAR-ONLY  {name}  ({len(bo)} instructions, {moved} diff lines, all of them s_*)")
            continue
        bad += 1
        print(f"DIFFERS    {name}  ({len(bo)} -> {len(bn)} instructions, {moved} diff lines)")
        if len(ro) != len(rn):  # (a line on one side only: show both lists whole)
            print(f"           resources old: {ro}\n           resources new: {rn}")
        for a, b in zip(ro, rn):
            if a != b:
                print(f"           {a}  ->  {b}")
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {bad + scalar} not identical"
          + (f", {scalar} of them scalar-only" if scalar else ""))
    sys.exit(1 if bad or (scalar and not scalar_ok) else 0)


if __name__ == "__main__":
    main()
