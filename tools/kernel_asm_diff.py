"""Compare the gfx950 machine code of the kernels of two sets of device-only compiles, kernel by kernel.

    hipcc <FLAGS of grafx_amd/build.py> -I <gendir> --offload-device-only -S csrc/X.hip -o X.s     (for every file)
    python tools/kernel_asm_diff.py --before old/*.s --after new/*.s [--removed dyn_bwd_a_kernel ...] [--renamed OLD=NEW ...]

For a change that moves kernels between translation units without touching them: every kernel is cut out of the
compiler's assembly (its label to its .Lfunc_end, the .amdhsa_kernel descriptor included), what depends only on its
position in a file is normalised (the numbers in local labels; comments, .p2align padding and the switch back to the text
section are dropped) and the
pieces are compared by mangled name.  A device function that is NOT inlined lies outside every such piece: the tool
names the ones it finds, they have to be compared by hand.  --renamed OLD=NEW (substrings of mangled names) replaces OLD by
NEW throughout the bodies before, for a kernel whose name changes with nothing else.  Exit status 0 when the kernels after
are the kernels before minus those named by --removed (substrings of the mangled name), no kernel is emitted by two files
after (a kernel emitted twice BEFORE is reported, and fails only when its copies differ: the comparison stands on either), and
every remaining one is identical.  Reads compiler output only.
"""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+")    # .LBB<n>_, .Lfunc_end<n>, .Ltmp<n>: <n> counts the functions of the file
COMMENT = re.compile(r"\s*;.*$")             # (loop comments quote those numbers and are padded to the label's width)


def kernels(paths, renamed=()):
    out, dup, split = {}, [], []
    for path in paths:
        lines = open(path).read().split("\n")
        names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
        start = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith("_") and l.split(":")[0] in names}
        for fn in (m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m):
            if fn not in names:
                print(f"WARNING      {path}: device function {fn} is not a kernel and is NOT compared")
        for name in names:
            if name not in start:
                sys.exit(f"{path}: kernel {name} has a descriptor but no label: not compiler output of the expected form")
            i = start[name]
            j = next(k for k in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
            body = [LOCAL.sub(r".L\1#", COMMENT.sub("", l)) for l in lines[i:j]]
            # (.text / .section .text.<name>,comdat after the descriptor: a template's instance and a plain kernel differ in it)
            body = [l for l in body if l.strip() and not re.match(r"\s*(\.p2align|\.text$|\.section\s+\.text\.)", l)]
            for a, b in renamed:
                name, body = name.replace(a, b), [l.replace(a, b) for l in body]
            if name in out:
                dup.append(name)
                if out[name] != body:
                    split.append(name)
            out[name] = body
    return out, dup, split


def figures(body):
    f = {"insts": sum(1 for l in body if re.match(r"\t[a-z]+_\w+", l))}
    for l in body:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|"
                     r"private_segment_fixed_size)\s+(\S+)", l)
        if m:
            f[m.group(1)] = m.group(2)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--removed", nargs="*", default=[])
    ap.add_argument("--renamed", nargs="*", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    old, dup_old, split_old = kernels(a.before, [r.split("=", 1) for r in a.renamed])
    new, dup_new, _ = kernels(a.after)
    gone = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    unexpected = [n for n in gone if not any(r in n for r in a.removed)]
    same = [n for n in old if n in new and old[n] == new[n]]
    differ = [n for n in old if n in new and old[n] != new[n]]
    print(f"kernels before {len(old)}, after {len(new)}; identical {len(same)}, differing {len(differ)}, "
          f"removed {len(gone)}, added {len(added)}, emitted twice before {len(dup_old)}, after {len(dup_new)}")
    for n in gone:
        print(("removed      " if n not in unexpected else "MISSING      ") + n)
    for n in added:
        print("ADDED        " + n)
    for n in dup_old:
        print(("emitted twice before " if n not in split_old else "EMITTED TWICE before, copies differ ") + n)
    for n in dup_new:
        print("EMITTED TWICE " + n)
    for n in differ:
        print(f"DIFFERS      {n}\n    before {figures(old[n])}\n    after  {figures(new[n])}")
    return 1 if (unexpected or added or differ or split_old or dup_new) else 0


if __name__ == "__main__":
    sys.exit(main())
