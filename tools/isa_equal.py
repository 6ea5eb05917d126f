#!/usr/bin/env python3
"""Compare two device assembly files (hipcc -S --cuda-device-only) kernel by kernel: one line per kernel of the OLD file,
SAME / DIFF / GONE, then the kernels only the NEW file has and the counts.  A kernel's body runs from its symbol line to
.end_amdhsa_kernel (instruction text and the .amdhsa_* resource lines); before comparing, the kernel's own mangled name is
replaced, `;` comments are stripped and the function index is dropped from .LBB<n>_ / .Lfunc_end<n> labels.
usage: isa_equal.py old.s new.s [--rename OLD=NEW ...] [--rename-re PATTERN=REPL ...] [--allow DIRECTIVE ...] [--dump DIR]
  --rename  literal substring of an old mangled name and what stands in its place in the new file (template lists that changed);
            the first one that matches a name is applied
  --rename-re  the same with a regular expression (re.sub); every one is applied, in the order given, after --rename
  --allow   an .amdhsa_* directive whose value may differ (reported next to SAME), e.g. .amdhsa_kernarg_size
  --dump    write the normalised bodies of differing kernels to DIR/<n>.old / .new (for diff)"""
import os
import re
import sys


def kernels(path):
    """{mangled name: normalised body lines} of every kernel (a symbol with an .amdhsa_kernel block) of the file"""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        inner = name[2:] if name.startswith("_Z") else name   # as it appears inside the names of the kernel's static objects
        body = []
        for ln in lines[start:end + 1]:
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            ln = ln.replace(name, "<kernel>").replace(inner, "<kernel>")
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
            body.append(ln)
        out[name] = body
    return out


def main(argv):
    renames, renames_re, allow, dump, files = [], [], [], None, []
    it = iter(argv)
    for a in it:
        if a == "--rename":
            renames.append(next(it).split("=", 1))
        elif a == "--rename-re":
            renames_re.append(next(it).split("=", 1))
        elif a == "--allow":
            allow.append(next(it))
        elif a == "--dump":
            dump = next(it)
        else:
            files.append(a)
    old, new = kernels(files[0]), kernels(files[1])
    seen, counts = set(), dict(SAME=0, DIFF=0, GONE=0)
    for n, (name, body) in enumerate(old.items()):
        to = name
        for a, b in renames:
            if a in to:
                to = to.replace(a, b)
                break
        for a, b in renames_re:
            to = re.sub(a, b, to)
        if to not in new:
            counts["GONE"] += 1
            print(f"GONE  {name}")
            continue
        seen.add(to)
        other, notes = new[to], []
        if len(body) == len(other):
            for i, (x, y) in enumerate(zip(body, other)):
                d = x.split()[0] if x.split() else ""
                if x != y and d in allow and d == y.split()[0]:
                    notes.append(f"{d} {x.split()[1]} -> {y.split()[1]}")
                    other = other[:i] + [x] + other[i + 1:]
        verdict = "SAME" if body == other else "DIFF"
        counts[verdict] += 1
        print(f"{verdict}  {name}" + (f" -> {to}" if to != name else "") + (f"  ({'; '.join(notes)})" if notes else ""))
        if verdict == "DIFF" and dump:
            os.makedirs(dump, exist_ok=True)
            open(os.path.join(dump, f"{n}.old"), "w").write("\n".join(body) + "\n")
            open(os.path.join(dump, f"{n}.new"), "w").write("\n".join(other) + "\n")
    for name in new:
        if name not in seen:
            print(f"NEW   {name}")
    print(f"kernels: {len(old)} before, {len(new)} after; {counts['SAME']} SAME, {counts['DIFF']} DIFF, {counts['GONE']} GONE, "
          f"{len(new) - len(seen)} NEW")
    return 1 if counts["DIFF"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
