#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds of librsp.so (for refactors that
must not change the machine code).

    python tools/isa_diff.py OLD.so NEW.so        exit status 0 = identical

Reports kernel symbols present in only one library, kernels whose instruction lines differ and
kernels whose descriptor metadata (register counts, LDS / scratch / kernarg sizes, from the code
objects' notes) differs.  Everything after a function's last `s_endpgm` is alignment padding that
depends on what the linker placed next, and is ignored.
"""
import re
import sys

import isa_check

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size")


def trim(body):
    """The instruction lines up to and including the last s_endpgm."""
    ends = [i for i, s in enumerate(body) if s.startswith("s_endpgm")]
    return body[:ends[-1] + 1] if ends else body


def metadata(lib):
    """{kernel symbol: {key: value}} from the notes of every gfx950 code object of the library."""
    out = {}
    notes = isa_check.disassemble(lib, tool_args=("llvm-readelf", "--notes"))
    for block in re.split(r"\n  - (?=\.)", notes)[1:]:   # the entries of amdhsa.kernels (their args sit deeper)
        block = "    " + block
        name = re.search(r"^    \.name:\s*(\S+)", block, re.M).group(1)
        out[name] = {k: re.search(r"^    %s:\s*(\S+)" % re.escape(k), block, re.M).group(1) for k in META}
    return out


def diff(old_fns, new_fns, old_meta, new_meta):
    """Lines describing every difference between two parsed libraries ([] = identical kernels)."""
    probs = ["only in OLD: " + k for k in sorted(set(old_meta) - set(new_meta))]
    probs += ["only in NEW: " + k for k in sorted(set(new_meta) - set(old_meta))]
    for k in sorted(set(old_meta) & set(new_meta)):
        a, b = trim(old_fns.get(k, [])), trim(new_fns.get(k, []))
        if a != b:
            i = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            probs.append("instructions differ: %s (%d vs %d lines, first at %d: %r vs %r)"
                         % (k, len(a), len(b), i, a[i:i + 1], b[i:i + 1]))
        if old_meta[k] != new_meta[k]:
            probs.append("descriptor differs: %s %s vs %s" % (k, old_meta[k], new_meta[k]))
    return probs


def load(lib):
    return isa_check.functions(isa_check.disassemble(lib)), metadata(lib)


def main():
    (of, om), (nf, nm) = load(sys.argv[1]), load(sys.argv[2])
    probs = diff(of, nf, om, nm)
    print("\n".join(probs + ["isa_diff: %d kernels in OLD, %d in NEW, %d differences" % (len(om), len(nm), len(probs))]))
    return 1 if probs or not om else 0


if __name__ == "__main__":
    sys.exit(main())
