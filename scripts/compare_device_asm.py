#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) of one translation unit as text:
the functions between the `-- Begin function` / `-- End function` markers, each kernel's
.amdhsa_kernel block and its .amdgpu_metadata entry, keyed by symbol, ignoring their order in the
file and the lines that name the per-compile __hip_cuid_ symbol.

    compare_device_asm.py OLD.s NEW.s      exit 0 and "IDENTICAL n kernels, m functions" if equal
    compare_device_asm.py --allow-new OLD.s NEW.s
                                           NEW may hold further kernels and functions (a change that adds
                                           variants under their own symbols); everything in OLD must be
                                           in NEW, equal.  Labels carry the function's ordinal in the file
                                           (.LBB12_3, .Lfunc_end12), which moves when functions are added:
                                           the ordinal and the comments that repeat it are left out of the
                                           comparison in this mode.
"""
import re
import sys


def pieces(path, strip_ordinals=False):
    text = "".join(l for l in open(path) if "__hip_cuid_" not in l)
    if strip_ordinals:
        text = re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+", r"\1", text)
        text = re.sub(r"[ \t]+;", " ;", text)   # the comment column moves with the label's width
    out = {}
    for m in re.finditer(r"-- Begin function (\S+)\n(.*?)-- End function", text, re.S):
        out["fn " + m.group(1)] = m.group(2)
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        out["hsa " + m.group(1)] = m.group(2)
    # a failed compile leaves an empty or truncated file: never a pass
    if not any(k.startswith("hsa ") for k in out) or ".end_amdgpu_metadata" not in text:
        sys.exit(f"{path}: no kernels or no metadata (did the compile fail?)")
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    for ent in re.split(r"\n  - (?=\.\w+:)", meta.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0]):
        name = re.search(r"\.symbol:\s+(\S+)", ent)
        if name:
            lines = sorted(l.strip(" -") for l in ent.splitlines())   # the first key carries the list dash
            out["meta " + name.group(1)] = "\n".join(lines)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--allow-new"]
    allow_new = len(args) != len(sys.argv) - 1
    old, new = pieces(args[0], allow_new), pieces(args[1], allow_new)
    bad = [k for k in sorted(set(old) | set(new)) if old.get(k) != new.get(k) and not (allow_new and k not in old)]
    for k in bad:
        print(("DIFFERS " if k in old and k in new else "ONLY IN OLD " if k in old else "ONLY IN NEW ") + k)
    if not bad:
        print(f"IDENTICAL {sum(k.startswith('hsa ') for k in old)} kernels, "
              f"{sum(k.startswith('fn ') for k in old)} functions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
