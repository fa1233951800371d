#!/usr/bin/env python3
"""Did a source change move a kernel's code?  Compares the gfx950 kernels of
two libdal.so builds by their disassembly (isa_stats.py's extraction).

usage: scripts/isa_diff.py LIB_A LIB_B [--kernel SUBSTR]

One line per kernel: identical, or differs with both builds' instruction
counts; kernels present in one build only are listed as such.  Addresses,
encodings, the symbol names of branch and call targets and the pc-relative
distance to a callee (s_getpc_b64 + s_add_u32 / s_addc_u32) are left out of
the comparison, so a kernel that merely moved inside the code object, or whose
out-of-line callee was renamed or moved, still reads identical.  Registers, scratch and
LDS are not here: they are in the code-object metadata (llvm-readelf --notes
on the extracted code object).  Exit status 1 when anything differs."""
import re
import sys

from isa_stats import object_functions


def instructions(body):
    """The instruction stream of one disassembled function: mnemonic and
    operands per line, without the address/encoding comment and without
    <symbol+off> annotations."""
    out = []
    pcrel = 0  # lines left of an s_getpc_b64 / s_add_u32 / s_addc_u32 address computation
    for line in body.splitlines()[1:]:
        text = line.split("//")[0].strip()
        if not text or text.endswith(":"):
            continue
        text = re.sub(r"\s*<[^>]*>", "", text)
        if text.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and text.startswith(("s_add_u32", "s_addc_u32")):
            # the distance to another function of the code object, not code
            text = re.sub(r",\s*[^,]+$", ", <pcrel>", text)
            pcrel -= 1
        else:
            pcrel = 0
        out.append(text)
    return out


def kernels(lib, sub):
    """Keyed by (code object, name): file-local helpers of two sources may share a name."""
    return {f"[{obj:2d}] {name}": instructions(body) for obj, name, body in object_functions(lib) if sub in name}


def main():
    args = sys.argv[1:]
    sub = ""
    if "--kernel" in args:
        i = args.index("--kernel")
        sub = args[i + 1]
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = (kernels(lib, sub) for lib in args)
    same = diff = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {args[0] if name in a else args[1]}: {name}")
            diff += 1
        elif a[name] == b[name]:
            print(f"identical {len(a[name]):7d}          {name}")
            same += 1
        else:
            print(f"DIFFERS   {len(a[name]):7d} {len(b[name]):7d}  {name}")
            diff += 1
    print(f"{same} identical, {diff} differ or unmatched ({args[0]} vs {args[1]})")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
