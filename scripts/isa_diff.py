#!/usr/bin/env python3
"""Per-kernel comparison of gfx950 device assembly: did a refactor change the instructions?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S old/gemm.hip -o old.s      (the Makefile's flags)
    hipcc ...                                                        -S csrc/gemm.hip -o gemm.s
    hipcc ...                                                        -S csrc/skinny.hip -o skinny.s
    python scripts/isa_diff.py old.s gemm.s skinny.s

The first file is the yardstick; the others together are the new build (a symbol may have moved between units).  Every
function symbol is cut out, comments, directives and the function number inside .LBBn_m labels are dropped, and the
instruction lists are compared.  Prints one markdown table row per symbol (instructions old / new, SAME / DIFF / GONE / NEW;
for a DIFF the VGPR / AGPR / SGPR / LDS / scratch figures of both sides from the .amdhsa_ block).  Exit status 1 unless
every symbol of the first file is SAME.
"""
import re
import sys


def parse(path):
    funcs, res, cur, kern = {}, {}, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            kern = res.setdefault(m.group(1), {})
        elif s == ".end_amdhsa_kernel":
            kern = None
        elif kern is not None and s.startswith(".amdhsa_"):
            k, _, v = s.partition(" ")
            kern[k[len(".amdhsa_"):]] = v.strip()
        m = re.match(r"\.type\s+([^,\s]+),@function", s)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and s and (s.startswith(".LBB") or not (s.startswith(".") or s.endswith(":"))):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))          # instructions and block labels; no directives, no symbol labels
    return funcs, res


def regs(r):
    if not r:
        return "-"
    total, acc = int(r.get("next_free_vgpr", 0)), int(r.get("accum_offset", 0))
    agpr = total - acc if acc and total > acc else 0
    return "v%d a%d s%d lds%s scr%s" % (total - agpr, agpr, int(r.get("next_free_sgpr", 0)),
                                         r.get("group_segment_fixed_size", "0"), r.get("private_segment_fixed_size", "0"))


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old_f, old_r = parse(sys.argv[1])
    new_f, new_r = {}, {}
    for p in sys.argv[2:]:
        f, r = parse(p)
        new_f.update(f)
        new_r.update(r)
    bad = 0
    print("| symbol | old | new | result | registers old -> new |")
    print("|---|---|---|---|---|")
    for name in sorted(set(old_f) | set(new_f)):
        o, n = old_f.get(name), new_f.get(name)
        verdict = "GONE" if n is None else "NEW" if o is None else "SAME" if o == n else "DIFF"
        bad += verdict in ("GONE", "DIFF")
        extra = "%s -> %s" % (regs(old_r.get(name)), regs(new_r.get(name))) if verdict == "DIFF" else ""
        count = lambda body: "-" if body is None else sum(not x.endswith(":") for x in body)
        print("| `%s` | %s | %s | %s | %s |" % (name, count(o), count(n), verdict, extra))
    print("\n%d symbols in %s, %d in the new build, %d not SAME" % (len(old_f), sys.argv[1], len(new_f), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
