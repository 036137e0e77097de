#!/usr/bin/env python3
"""Instructions one wave executes along a path through a kernel's gfx950 assembly (hipcc ... --cuda-device-only -S).

    python tools/count_isa_path.py <file.s> <kernel name substring> <block>[*<times>] ...

A block is a label of the kernel (".LBB72_153" or "LBB72_153") or "<label>+<k>" for the k-th unlabelled fall-through
block after it ("; %bb.N" comment lines start one); it ends at the next label or block comment.  Prints, per block and
for the whole path, VALU (v_*), SALU (s_* without waits, nops and barriers), LDS (ds_*), exec-mask writes
(s_and_saveexec / s_andn2 / s_or / s_mov with exec as destination) and s_nop counts, each times its multiplier.  The
path is the reader's: the blocks a wave of the given degrees runs through and how often (profiles/r08_compiler_report.txt
lists the ones it counted)."""
import re
import sys

path, kernel = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and kernel in l.split(":")[0] and l.rstrip().split(";")[0].rstrip().endswith(":"))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
blocks, name, sub = {}, "entry", 0
for l in lines[start + 1:end]:
    t = l.strip()
    m = re.match(r"^(\.LBB\d+_\d+):", t)
    if m:
        name, sub = m.group(1), 0
        continue
    if t.startswith("; %bb."):
        sub += 1
        continue
    if not t or t.startswith(";") or t.startswith("."):
        continue
    blocks.setdefault(f"{name}+{sub}" if sub else name, []).append(t.split(";")[0].strip())


def classify(ins):
    op = ins.split()[0]
    c = {"valu": 0, "salu": 0, "lds": 0, "exec": 0, "nop": 0}
    if op == "s_nop":
        c["nop"] = 1
    elif op.startswith("v_"):
        c["valu"] = 1
    elif op.startswith("ds_"):
        c["lds"] = 1
    elif op.startswith("s_") and op not in ("s_waitcnt", "s_barrier"):
        c["salu"] = 1
        if re.match(r"s_(and_saveexec|andn2|or|mov|and|xor)\w*\s+exec\b", ins) or op.startswith("s_and_saveexec"):
            c["exec"] = 1
    return c


total = {"valu": 0, "salu": 0, "lds": 0, "exec": 0, "nop": 0}
for spec in sys.argv[3:]:
    label, _, times = spec.partition("*")
    times = int(times) if times else 1
    label = label if label.startswith(".") else "." + label
    if label not in blocks:
        sys.exit(f"no block {label} in the kernel")
    c = {k: 0 for k in total}
    for ins in blocks[label]:
        for k, v in classify(ins).items():
            c[k] += v
    print(f"{label:>16} x{times:<3}" + "".join(f" {k} {c[k]:>3}" for k in c))
    for k in total:
        total[k] += times * c[k]
print(f"{'path':>16}     " + "".join(f" {k} {total[k]:>3}" for k in total))
