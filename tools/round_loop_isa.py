"""Static look at the Newton round loop of a sweep kernel (analysis build: tools/kernel_regs.sh <unit>.hip -DCADNIP_MARKS leaves the assembly in
/tmp/isa): instructions between the loop-top mark (17) and the loop-end mark (16) in layout order, both sides of every branch counted --
how many there are, how many reload a spilled SGPR (v_readlane from a register that v_writelane fills: the dense core's row broadcasts read
other registers) and how many are scalar loads (s_load: kernarg segment, block descriptors, pass words -- the base registers are copies, so
the assembly does not tell them apart), scratch instructions and s_waitcnt.

usage: python tools/round_loop_isa.py /tmp/isa/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s <mangled kernel name substring>"""
import collections
import re
import sys


def kernel_lines(path, kern):
    inside = False
    out = []
    for line in open(path):
        if not inside:
            inside = re.match(r"^\S*%s\S*:" % re.escape(kern), line) is not None
            continue
        t = line.strip()
        if t.startswith("s_endpgm"):
            break
        out.append(t)
    return out


def main():
    path, kern = sys.argv[1], sys.argv[2]
    lines = kernel_lines(path, kern)
    spill_regs = set()
    for t in lines:
        m = re.match(r"v_writelane_b32 (v\d+),", t)
        if m:
            spill_regs.add(m.group(1))
    marks = [(i, int(re.match(r"; @@MARK (\d+)", t).group(1))) for i, t in enumerate(lines) if t.startswith("; @@MARK")]
    lo = min(i for i, m in marks if m == 17)
    hi = max(i for i, m in marks if m == 16)
    c = collections.Counter()
    slots = set()
    for i, t in enumerate(lines):
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        op = t.split()[0]
        where = "loop" if lo <= i <= hi else "outside"
        c[where, "instr"] += 1
        m = re.match(r"v_readlane_b32 \S+ (v\d+), (\d+)", t)
        if m and m.group(1) in spill_regs:
            c[where, "reload"] += 1
            if where == "loop":
                slots.add((m.group(1), m.group(2)))
        if op == "v_writelane_b32":
            c[where, "spill_store"] += 1
        if op.startswith("s_load"):
            c[where, "s_load"] += 1
        if op.startswith("scratch_"):
            c[where, "scratch"] += 1
        if op == "s_waitcnt":
            c[where, "s_waitcnt"] += 1
    print("kernel %s: SGPR-spill registers %s" % (kern, " ".join(sorted(spill_regs, key=lambda r: int(r[1:])))))
    for where in ("loop", "outside"):
        print("  %-8s instructions %6d  v_readlane reloads %4d  v_writelane stores %4d  s_load %4d  scratch_* %3d  s_waitcnt %4d" % (
            where, c[where, "instr"], c[where, "reload"], c[where, "spill_store"], c[where, "s_load"], c[where, "scratch"], c[where, "s_waitcnt"]))
    print("  distinct spill slots reloaded in the loop: %d" % len(slots))


if __name__ == "__main__":
    main()
