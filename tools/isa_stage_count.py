#!/usr/bin/env python3
"""Instruction classes of a fused kernel's tile loop, segment by segment (the s_setprio markers the stages carry), from a device
assembly listing (tools/isa_lint.py device_asm, tools/kres.py).
  tools/isa_stage_count.py <listing.s | kind> <instantiation substring, e.g. ILb0ELi2ELi45ELi2ELb0ELb0> [--ops] [--smem]
<kind> (fast, mfma, exact) without a path compiles the unit with the flags of tools/isa_lint.py.
Only instructions in program order between the markers are counted: cold blocks the compiler moved behind the loop fall into the last segment.
Scalar loads are split by base register: `smem karg` reads the kernarg segment (the kernel's s[0:1], or a copy of it made with s_mov_b64 /
s_mov_b32 pairs is NOT followed: hipcc keeps the pointer where it arrives), `smem other` anything else (state, tables).  --smem lists them.
tests/test_tile_loop_smem.py uses segments() and kernarg_loads()."""
import collections
import os
import re
import sys

KARG_BASE = "s[0:1]"       # where the kernarg segment pointer arrives (no other user SGPR precedes it in these kernels: checked by kernarg_base)


def kernel_body(text, inst):
    """Lines of the one fmd_fused_kernel instantiation whose mangled name holds `inst`, label to s_endpgm."""
    m = re.search(r"^(_ZN\S*fmd_fused_kernel%s\S*):" % re.escape(inst), text, re.M)
    if not m:
        raise KeyError("no fmd_fused_kernel instantiation matches %r" % inst)
    body = text[m.end():]
    body = body[:body.index("s_endpgm")]
    return [l.split(";")[0].strip() for l in body.splitlines()]


def kernarg_base(text, inst):
    """The SGPR pair of the kernarg segment pointer, from the kernel descriptor's enabled user SGPRs (it is the first one enabled here)."""
    m = re.search(r"\.amdhsa_kernel \S*fmd_fused_kernel%s\S*\n(.*?)\.end_amdhsa_kernel" % re.escape(inst), text, re.S)
    if m:
        before = [k for k in ("private_segment_buffer", "dispatch_ptr", "queue_ptr")
                  if re.search(r"\.amdhsa_user_sgpr_%s\s+1" % k, m.group(1))]
        if before or not re.search(r"\.amdhsa_user_sgpr_kernarg_segment_ptr\s+1", m.group(1)):
            raise RuntimeError("the kernarg pointer is not the first user SGPR of %s: %s" % (inst, before))
    return KARG_BASE


def cls(op, rest=""):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "lds"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"): return "wait/nop"
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return "branch"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", rest)]
        return "smem karg" if len(ops) > 1 and ops[1] == KARG_BASE else "smem other"
    if op.startswith("s_"): return "salu"
    if op.startswith("buffer_") or op.startswith("global_") or op.startswith("scratch_"): return "vmem"
    return "other"


def segments(lines):
    """[(name, [(op, operands), ...])]: the code before the first s_setprio is 'prologue', then one segment per marker in program order
    ('prio 0', 'prio 1', ...; the fused kernels raise the priority twice to 3: stage D + flush, then the roll and everything behind the loop)."""
    segs, cur, name = [], [], "prologue"
    for l in lines:
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        parts = l.split(None, 1)
        op, rest = parts[0], parts[1] if len(parts) > 1 else ""
        if op == "s_setprio":
            segs.append((name, cur))
            cur, name = [], "prio " + rest.strip()
            continue
        cur.append((op, rest))
    segs.append((name, cur))
    return segs


def kernarg_loads(seg):
    """The scalar loads of a segment whose base is the kernarg pointer, as 'opcode offset' strings."""
    out = []
    for op, rest in seg:
        if cls(op, rest) == "smem karg":
            ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", rest)]
            out.append("%s %s" % (op, ops[2] if len(ops) > 2 else "?"))
    return out


def until_back_edge(seg, lines):
    """The part of the last segment that belongs to the loop: up to its first backward branch (the loop's back edge)."""
    labels = {}
    for no, l in enumerate(lines):
        if l.endswith(":"):
            labels[l[:-1]] = no
    # position of the segment's instructions in `lines`: walk from the last s_setprio
    start = max(no for no, l in enumerate(lines) if l.startswith("s_setprio"))
    out = []
    for no in range(start + 1, len(lines)):
        l = lines[no]
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        parts = l.split(None, 1)
        op, rest = parts[0], parts[1] if len(parts) > 1 else ""
        out.append((op, rest))
        if (op.startswith("s_cbranch") or op == "s_branch") and labels.get(rest.strip(), no) < start:
            break
    return out


def main(argv):
    src, inst = argv[1], argv[2]
    if not os.path.exists(src):
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import isa_lint
        src = isa_lint.device_asm(src)
    text = open(src).read()
    kernarg_base(text, inst)
    lines = kernel_body(text, inst)
    segs = segments(lines)
    for n, seg in segs:
        c = collections.Counter(cls(op, rest) for op, rest in seg)
        print("%-10s %s" % (n, dict(sorted(c.items()))), "sum", sum(c.values()))
    roll = until_back_edge(segs[-1][1], lines)
    c = collections.Counter(cls(op, rest) for op, rest in roll)
    print("%-10s %s" % ("(roll, to the back edge)", dict(sorted(c.items()))), "sum", sum(c.values()))
    if "--smem" in argv:
        for n, seg in segs[1:-1] + [("roll", roll)]:
            print(n, kernarg_loads(seg))
    if "--ops" in argv:
        for n, seg in segs:
            ops = collections.Counter(re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", op) for op, rest in seg if cls(op) == "valu")
            print(n, ops.most_common(14))


if __name__ == "__main__":
    main(sys.argv)
