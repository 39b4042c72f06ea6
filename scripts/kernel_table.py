#!/usr/bin/env python3
"""Per-kernel resource table of one HIP source, and its comparison with an earlier build of the same source.

  kernel_table.py NEW.s NEW.remarks [OLD.s OLD.remarks] [--match REGEX] [--csv OUT] [--rename REGEX=REPL ...]

NEW.s / OLD.s:       hipcc ... -S --cuda-device-only
NEW.remarks / OLD..: stderr of hipcc ... -Rpass-analysis=kernel-resource-usage

Prints one row per kernel whose demangled name matches REGEX (default: every kernel): VGPRs, scratch bytes per lane, occupancy
(waves per SIMD), number of device instructions; with an OLD build also the old figures and whether the opcode sequence (mnemonics
only: register numbering and label names may differ) is the same.  Kernels outside REGEX are only compared: the script ends with
status 1 when one of them changed its opcode sequence.  --rename rewrites the demangled names of the OLD build (re.sub) before the
two are paired, for kernels that changed their name or template arguments, e.g.
  --rename 'window_attention_long_kernel<(.*)>=window_attention_kernel<\1, 9>' 'window_attention_kernel<(\d, \w+)>$=window_attention_kernel<\1, 4>'"""
import argparse
import csv
import re
import subprocess
import sys

sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/i-vit_amd/csrc")
from check_resources import parse  # noqa: E402


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, (re.sub(r"^(void )?\(anonymous namespace\)::|\(.*\)$", "", d) for d in out.splitlines())))


def opcodes(path):
    """mangled kernel name -> list of instruction mnemonics"""
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur = kernels.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^\t([a-z][a-z0-9_]+)\b", line)
        if cur is not None and m:
            cur.append(m.group(1))
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--match", default=".")
    ap.add_argument("--csv")
    ap.add_argument("--rename", nargs="*", default=[])
    args = ap.parse_args()
    def load(s_path, remarks_path, renames=()):
        """demangled kernel name -> (resources, opcode list)"""
        ops, res = opcodes(s_path), parse(open(remarks_path, errors="replace").read())
        names = demangle(sorted(res))
        for r in renames:
            pat, repl = r.split("=", 1)
            names = {k: re.sub(pat, repl, v) for k, v in names.items()}
        return {names[k]: (res[k], ops[k]) for k in res}

    new = load(args.files[0], args.files[1])
    old = load(args.files[2], args.files[3], args.rename) if len(args.files) == 4 else {}
    rows, changed_outside = [], []
    for name in sorted(set(new) | set(old)):
        (n, n_ops), (o, o_ops) = new.get(name, (None, None)), old.get(name, (None, None))
        same = "" if not (n and o) else "same" if n_ops == o_ops else "differs"
        if not re.search(args.match, name):
            if same == "differs":
                changed_outside.append(name)
            continue
        f = lambda r, key: "" if r is None else r.get(key, "")
        rows.append([name, f(n, "VGPRs"), f(n, "Scratch"), f(n, "Occupancy"), len(n_ops) if n else "",
                     f(o, "VGPRs"), f(o, "Scratch"), f(o, "Occupancy"), len(o_ops) if o else "", same or ("new" if n else "gone")])
    head = ["kernel", "vgprs", "scratch", "occupancy", "instructions", "parent_vgprs", "parent_scratch", "parent_occupancy",
            "parent_instructions", "opcodes"]
    if args.csv:
        with open(args.csv, "w", newline="") as fh:
            csv.writer(fh).writerows([head] + rows)
    for r in [head] + rows:
        print(" ".join(str(x) for x in r))
    if changed_outside:
        print("opcode sequence changed outside --match:", ", ".join(changed_outside))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
