#!/usr/bin/env python3
"""Compare the device code of fmd_fused_kernel instantiations in two device-only assemblies of one translation unit
(hipcc -S --cuda-device-only with csrc/Makefile's flags): every instantiation of OLD must have an instruction-for-instruction identical
body in NEW (instructions and branch labels; directives and the kernel descriptor - whose kernarg size grows with the new parameter - are
not compared).  A template parameter added at the end (LV) appends ELb0E to the template arguments and a parameter to the signature;
names are compared with both stripped, and block / function labels are numbered by position, not by the file's order.  Two listings with the
same template parameters (a change that adds a kernel beside the fused one) are compared name for name.

    python3 tools/asm_body_diff.py old.s new.s      -> prints one line per differing or missing instantiation, exit 1 if any

--kernels REGEX compares the kernels whose mangled name the pattern is found in instead - every such kernel of OLD, name for name, the two
listings being of any units (a change that moves kernels from one translation unit to another):

    python3 tools/asm_body_diff.py --kernels 'fmd_(?!fused)\w+_kernel' old_fast.s new_recv.s
"""
import re
import sys

FUSED = r"^_ZN12_GLOBAL__N_116fmd_fused_kernel"      # the kernels compared without --kernels
LABEL = re.compile(r"^(\w+):\s*(?:;.*)?$", re.M)


def bodies(path, pattern):
    text = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\w+)", text, re.M))
    out = {}
    for m in LABEL.finditer(text):
        name = m.group(1)
        if name not in kernels or not re.search(pattern, name):
            continue
        end = text.index("s_endpgm", m.end())
        end = text.index("\n.Lfunc_end", end)
        lines = []
        for ln in text[m.end():end].splitlines():
            ln = ln.split(";", 1)[0].rstrip()
            st = ln.strip()
            if not st or (st.startswith(".") and not re.match(r"\.LBB\d+_\d+:", st)):   # directives and metadata: instructions and labels only
                continue
            lines.append(ln)
        labels = {}
        for ln in lines:
            for lab in re.findall(r"\.LBB\d+_\d+", ln):
                labels.setdefault(lab, ".L%d" % len(labels))
        body = "\n".join(re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], ln) for ln in lines)
        out[name] = body
    return out


def canonical(name):
    """the OLD spelling of a NEW name: the trailing LV = false argument and the level pointer of the signature removed"""
    name = re.sub(r"(fmd_fused_kernelILb[01]ELi\d+ELi\d+ELi\d+ELb[01])ELb0E", r"\1E", name)
    return name.replace("P15HIP_vector_typeIfLj2EE", "")


def main(argv):
    pattern = FUSED
    if len(argv) > 1 and argv[1] == "--kernels":
        pattern, argv = argv[2], argv[:1] + argv[3:]
    old, new = bodies(argv[1], pattern), bodies(argv[2], pattern)
    newc = {canonical(k): v for k, v in new.items() if re.search(r"ELb[01]ELb0EEEv", k)}
    newc.update(new)                      # the same spelling in both listings: name for name
    bad = 0
    for name, body in sorted(old.items()):
        if name not in newc:
            print("missing in new:", name)
            bad += 1
        elif newc[name] != body:
            print("body differs:", name)
            bad += 1
    return 1 if bad or not old else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
