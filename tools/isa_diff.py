#!/usr/bin/env python3
"""Compare the kept gfx950 ISA (csrc/*-gfx950.s) of two builds, unit by unit and kernel symbol by kernel symbol.

    tools/isa_diff.py <dir of the old build's .s> <dir of the new build's .s>

Comments, block labels and directives are stripped.  Per unit one verdict, the worst of its symbols:
  identical  the same instruction text and the same resource lines (register / LDS / scratch / spill counts, next_free_*)
  renamed    the same mnemonic sequence and the same resources (registers or labels renumbered)
  different  anything else: prints the change in the instruction count, the mnemonic histogram delta and the resource lines that
             changed, symbols that changed in the same way on one line
Exit status 1 if any unit is different.  It looks for no particular instruction."""
import collections, glob, os, re, sys

RES = re.compile(r"\.(vgpr_count|sgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|[sv]gpr_spill_count"
                 r"|amdhsa_next_free_[sv]gpr)\b:?\s*(\S+)")


def parse(text):
    """-> {symbol: (instruction lines, sorted resource lines)}"""
    code, cur = {}, None
    funcs = set(re.findall(r"\.type\s+(\S+),@function", text))
    for raw in text.splitlines():
        line = raw.split(";")[0].rstrip()
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in funcs:  # (block labels start with '.')
            cur = m.group(1)
            code[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and line[:1] in " \t" and not line.lstrip().startswith(".") and line.strip():
            code[cur].append(" ".join(line.split()))
    res = collections.defaultdict(set)
    # the kernel descriptor's block and the kernel's entry in the metadata (a YAML list item with a .name at its own level)
    blocks = [(m.group(1), m.group(2)) for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S)]
    for item in re.split(r"\n  - (?=\.)", text.partition("amdhsa.kernels:")[2].partition(".end_amdgpu_metadata")[0]):
        m = re.search(r"\n    \.name:\s+(\S+)", "\n" + item)
        if m:
            blocks.append((m.group(1), item))
    for name, body in blocks:
        res[name].update("%s %s" % r.groups() for r in RES.finditer(body))
    return {s: (ins, sorted(res.get(s, ()))) for s, ins in code.items()}


def compare(old, new):
    """-> (verdict, report lines) for two texts of one unit; symbols that changed in the same way share a report line"""
    a, b = parse(old), parse(new)
    verdict, how = "identical", collections.defaultdict(list)
    for s in sorted(set(a) | set(b)):
        if s not in a or s not in b:
            how["only in the %s build" % ("old" if s in a else "new")].append(s)
            continue
        (ia, ra), (ib, rb) = a[s], b[s]
        ma, mb = [i.split()[0] for i in ia], [i.split()[0] for i in ib]
        if ma != mb or ra != rb:
            ha, hb = collections.Counter(ma), collections.Counter(mb)
            d = ["%+d %s" % (hb[k] - ha[k], k) for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]]
            if ma != mb and not d:
                d = ["same mnemonics in another order"]
            d += ["%s -> %s" % (x, y.split()[-1]) for x, y in zip(ra, rb) if x != y] if len(ra) == len(rb) else ["resource lines %s -> %s" % (ra, rb)]
            how["%+d instructions: %s" % (len(ib) - len(ia), ", ".join(d))].append(s)
        elif ia != ib and verdict == "identical":
            verdict = "renamed"
    out = ["  %d symbol%s, e.g. %s (%d instructions before): %s" % (len(v), "s"[:len(v) > 1], v[0], len(a.get(v[0], b.get(v[0]))[0]), k)
           for k, v in how.items()]
    return ("different" if how else verdict), out


def main(old_dir, new_dir):
    worst = 0
    units = lambda d: {os.path.basename(p).split("-hip-")[0]: p for p in glob.glob(os.path.join(d, "*-gfx950.s"))}
    uo, un = units(old_dir), units(new_dir)
    for u in sorted(set(uo) | set(un)):
        if u not in uo or u not in un:
            verdict, out = "different", ["  unit only in the %s build" % ("old" if u in uo else "new")]
        else:
            verdict, out = compare(open(uo[u]).read(), open(un[u]).read())
        print("%-22s %s" % (u, verdict))
        print("\n".join(out), end="\n" if out else "")
        worst |= verdict == "different"
    return worst


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
