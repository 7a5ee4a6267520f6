#!/usr/bin/env python3
"""Compare device assembly files function by function (hipcc <library flags> --cuda-device-only -S unit.hip -o x.s).

    tools/isa_diff.py [--rename OLD=NEW ...] parent.s [move.s ...] final.s

Every file after the first is compared against the FIRST.  Per function: instruction counts, the resource table of a
kernel (VGPR, SGPR, LDS bytes, private segment bytes, SGPR / VGPR spills) and SAME or DIFF; for DIFF a unified diff of the
instruction streams.  An instruction stream is what lies between the function's label and its end label without comments,
directives and blank lines; branch-target labels are renumbered in order of appearance, so only addresses and label
numbers may differ between two streams that compare SAME.  Exit status 1 if anything differs.

Functions are paired by name.  --rename OLD=NEW pairs the first file's OLD with NEW in the others; both are names as the
first column prints them, without a leading "void " (--rename 'k_ingest_area<PackedSrc>=k_area<true, PackedSrc>').
"""
import difflib
import re
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count",
        ".vgpr_spill_count")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"\(anonymous namespace\)::|\(.*", "", d) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    funcs, meta, cur, entry, prev = {}, {}, None, {}, ""
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        m = re.match(r"(\w+):", line)
        if m and cur is None and re.match(r"\s+\.type\s+%s,@function" % re.escape(m.group(1)), prev):
            cur = m.group(1)
            funcs[cur] = []
        elif cur and re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        elif cur and line.strip() and not line.strip().startswith("."):
            funcs[cur].append(line.strip())
        elif cur and re.match(r"\.LBB\d+_\d+:", line):
            funcs[cur].append(line.strip())
        if re.match(r"  - \.", line):            # a kernel's metadata entry begins; its own keys sit at four spaces
            entry = {}
        m = re.match(r"(?:    |  - )(\.\w+):\s+(\S+)", line)
        if m and m.group(1) == ".name":
            meta[m.group(2)] = entry
        elif m and m.group(1) in META:
            entry[m.group(1)] = int(m.group(2))
        prev = raw
    for name, body in funcs.items():          # renumber the branch targets in order of appearance
        order = {}
        for ln in body:
            for lb in re.findall(r"\.LBB\d+_\d+", ln):
                order.setdefault(lb, ".L%d" % len(order))
        funcs[name] = [re.sub(r"\.LBB\d+_\d+", lambda m: order[m.group(0)], ln) for ln in body]
    return funcs, meta


def count(body):
    return sum(1 for ln in body if not ln.endswith(":"))


def table(meta):
    return "-" if not meta else "v%d s%d lds%d priv%d spill%d/%d" % tuple(meta.get(k, 0) for k in META)


def bare(name):
    return name[5:] if name.startswith("void ") else name


def main(paths, renames):
    parsed = [parse(p) for p in paths]
    base_f, base_m = parsed[0]
    names = demangle(list(base_f))
    by_name = [{bare(d): n for n, d in demangle(list(f)).items()} for f, _ in parsed[1:]]
    paired = [set() for _ in parsed[1:]]
    differs = False
    for fn in base_f:
        cols, diffs = ["%d %s" % (count(base_f[fn]), table(base_m.get(fn)))], []
        new = renames.get(bare(names[fn]))
        for k, (path, (f, m)) in enumerate(zip(paths[1:], parsed[1:])):
            other = by_name[k].get(new, fn) if new else fn      # a file from before the rename still has the old name
            if other not in f:
                cols.append("MISSING"); differs = True
                continue
            paired[k].add(other)
            same = f[other] == base_f[fn] and m.get(other) == base_m.get(fn)
            cols.append("%d %s %s" % (count(f[other]), table(m.get(other)), "SAME" if same else "DIFF"))
            if not same:
                differs = True
                diffs.append((path, list(difflib.unified_diff(base_f[fn], f[other], paths[0], path, n=0, lineterm=""))))
        print("%-28s | %s" % (names[fn] + (" -> " + new if new else ""), " | ".join(cols)))
        for path, d in diffs:
            for ln in d:
                print("    " + ln)
    for k, (path, (f, m)) in enumerate(zip(paths[1:], parsed[1:])):
        for fn in f:
            if fn not in paired[k]:
                print("%-28s | only in %s: %d" % (fn, path, count(f[fn]))); differs = True
    return 1 if differs else 0


if __name__ == "__main__":
    args, renames, it = [], {}, iter(sys.argv[1:])
    for a in it:
        if a != "--rename":
            args.append(a)
            continue
        pair = next(it, "")
        if "=" not in pair:
            sys.exit("isa_diff.py: --rename takes OLD=NEW, got %r" % pair)
        old, new = pair.split("=", 1)
        renames[bare(old)] = bare(new)
    if len(args) < 2:
        sys.exit(__doc__)
    sys.exit(main(args, renames))
