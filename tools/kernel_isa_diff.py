#!/usr/bin/env python3
"""Are the gfx950 instructions of two builds of the library the same, function by function?

    python tools/kernel_isa_diff.py old/librvdd_hip.so new/librvdd_hip.so      # exit 1 if anything differs

For a change that moves kernels between translation units or renames their scope and claims to leave the code alone.
Every function of every code object is disassembled (llvm-objdump -d) and keyed by its demangled name without
`(anonymous namespace)::`; addresses, the trailing `//` comment (address and encoding) and the alignment padding behind a
function's last instruction are dropped, since those depend on where the function lies in its code object.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects  # noqa: E402

PAD = ("s_nop", "s_code_end", "...")      # "...": objdump's run of zero words


def functions(lib):
    """-> {demangled name: [instruction text, ...]} over all code objects of the library."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", co], capture_output=True, text=True,
                                  check=True).stdout
            cur = None
            for ln in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
                if m:
                    name = m.group(1).replace("(anonymous namespace)::", "")
                    if name in out:
                        raise SystemExit(f"{lib}: two functions named {name}")
                    cur = out[name] = []
                elif cur is not None and ln.startswith(("\t", " ")) and ln.strip():
                    cur.append(" ".join(ln.split("//")[0].split()))
    for ins in out.values():
        while ins and ins[-1].startswith(PAD):
            ins.pop()
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"only in {'old' if name in old else 'new'}: {name}")
            bad += 1
        elif old[name] != new[name]:
            first = next((i for i, (a, b) in enumerate(zip(old[name], new[name])) if a != b), min(len(old[name]), len(new[name])))
            print(f"differs: {name}: {len(old[name])} -> {len(new[name])} instructions, first difference at {first}")
            bad += 1
    print(f"{len(old)} functions old, {len(new)} new, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
