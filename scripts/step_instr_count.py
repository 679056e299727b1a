#!/usr/bin/env python3
"""Instructions per trellis step of the exact decoder's three hot loop bodies, counted offline in the
ISA of the product library (no GPU).

    step_instr_count.py [LIB] [--kernel MANGLED] [--kw 15] [--json OUT] [--dump DIR]

LIB defaults to turbo_decoder_cuda_amd/libturbo_mi355x.so as build() leaves it.  The library's device
code objects are taken out with `llvm-objdump --offloading` (on a copy in a temporary directory), the
one that defines the kernel is disassembled, and the kernel (default: turbo_decode_kernel<double, 0>,
fp64 log-MAP, bench.py's config 2) is cut into straight-line regions: a region ends at every branch,
at every branch target and at every s_barrier.  The script only classifies and counts instructions
by the prefix of their mnemonic; it looks for no particular instruction beyond the anchors below.

Anchoring (survives recompilation: it uses what the source pins, not addresses or registers).
A max* TABLE-ROW READ is the pair the table layout fixes (td_kernels.hip, lut_fields): one
ds_read2_b64 with offset1:16 (thr and v[q], 128 B apart) and one ds_read_b64 with offset:384 (v[q+1])
of the same address register.  Every scheduled step pins its row read between scheduling barriers, so
an unrolled window is a straight-line region with exactly kW row reads:
  alpha   kW row reads and kW global stores carrying `nt` (astore_row's scheduled alpha rows; the
          committed-order redo window, alpha_window, stores without nt) -- AlphaSchedS, kASpec path.
  beta    kW row reads, kW or more ds_write_b64 (the step's beta publish) and no global store --
          BetaSched.  The kernel holds more than one instance (the B pass's first and steady-state
          windows); each is listed, the summary takes the mean.
  fold    14 row reads (7 max* of each of the two E_seq folds of one item), at least the 8
          ds_read_b128 of the item's alpha and beta blocks and no LDS write mark a fold body.  The
          item's stores sit under lane masks, which the compiler turns into s_cbranch_execz skips, and
          the window's barrier may sit at the loop's head (rotated loop), so a fold is counted as its
          whole per-window LOOP: from the lowest target of the backward branches found between the
          body and the next fold body, through the last of those branches -- every instruction a
          fold wave issues per window when no skip is taken, barrier and slot counters included.
          fold_item_fast, the full windows' body, is the loop with at most two global stores (the
          extrinsic and the decision).  The generic fold_item's loop also stores the raw LLR and the
          Le dump (fold_generic), and its copies for a SISO's first two folded windows are peeled
          (no backward branch: fold_peeled); both are listed outside the summary.  One item per lane
          and window, so a fold wave's cost per trellis step is the loop's count divided by kW.
A window region includes the window's own prologue and epilogue (first operand reads, the miss
ballot, pointer bumps): those are issued once per kW steps and are part of the per-step cost.

Classes: valu (v_*), salu (s_* arithmetic, moves, compares, branches), lds (ds_*), global (global_*,
buffer_*, flat_*, scratch_*), wait (s_waitcnt*, s_nop, v_nop, s_sleep), other (s_barrier, s_setprio,
scalar loads, ...).  `dpp` (v_*_dpp) is reported beside them as a sub-count of valu.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
KERNEL = "_ZN2td19turbo_decode_kernelIdLi0EEEvNS_12DecodeParamsIT_EE"
CLASSES = ("valu", "salu", "lds", "global", "wait", "other")


def classify(mn: str) -> str:
    if mn in ("s_nop", "v_nop", "s_sleep") or mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "global"
    if mn.startswith(("s_load", "s_buffer_load", "s_barrier", "s_setprio", "s_memtime", "s_memrealtime",
                      "s_endpgm", "s_sethalt", "s_setreg", "s_getreg", "s_icache", "s_dcache_inv")):
        return "other"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def disassemble(lib: str, kernel: str) -> str:
    objdump = os.path.join(LLVM, "llvm-objdump")
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, copy)
        subprocess.check_call([objdump, "--offloading", copy], stdout=subprocess.DEVNULL)
        for co in sorted(glob.glob(copy + ".*amdgcn*")):
            syms = subprocess.check_output([objdump, "-t", co], text=True)
            if re.search(rf"\sF\s+\.text\s+\S+\s+(\.protected\s+)?{re.escape(kernel)}$", syms, re.M):
                return subprocess.check_output(
                    [objdump, "-d", "--no-show-raw-insn", f"--disassemble-symbols={kernel}", co], text=True)
    sys.exit(f"{lib}: no device code object defines {kernel}")


LINE = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
TARGET = re.compile(r"<[^>]*\+0x([0-9a-fA-F]+)>")


def parse(text: str):
    """[(address, mnemonic, operands)] and {branch address: target address}."""
    ins, base, targets = [], None, {}
    for line in text.splitlines():
        m = LINE.match(line)
        if not m:
            continue
        mn, ops, addr = m.group(1), m.group(2), int(m.group(3), 16)
        if base is None:
            base = addr
        ins.append((addr, mn, ops))
        if mn.startswith(("s_cbranch", "s_branch")):
            t = TARGET.search(line)
            if t:
                targets[addr] = base + int(t.group(1), 16)
    return ins, targets


def regions(ins, branches):
    targets = set(branches.values())
    out, cur = [], []
    for addr, mn, ops in ins:
        if addr in targets and cur:
            out.append(cur)
            cur = []
        cur.append((addr, mn, ops))
        if mn.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_setpc", "s_swappc")):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def features(reg):
    f = dict(row2=0, row1=0, nt_store=0, gstore=0, b128=0, w64=0)
    for _, mn, ops in reg:
        if mn == "ds_read2_b64" and re.search(r"offset1:16\b", ops) and "offset0" not in ops:
            f["row2"] += 1
        elif mn == "ds_read_b64" and re.search(r"offset:384\b", ops):
            f["row1"] += 1
        elif mn.startswith("global_store"):
            f["gstore"] += 1
            if re.search(r"\bnt\b", ops):
                f["nt_store"] += 1
        elif mn == "ds_read_b128":
            f["b128"] += 1
        elif mn == "ds_write_b64":
            f["w64"] += 1
    f["rows"] = min(f["row2"], f["row1"])
    return f


def count(reg, per):
    c = {k: 0 for k in CLASSES}
    dpp = 0
    for _, mn, _ops in reg:
        c[classify(mn)] += 1
        dpp += mn.endswith("_dpp")
    total = len(reg)
    return {
        "address": f"{reg[0][0]:#x}", "instructions": total, "divided_by": per,
        "per_step": {**{k: round(v / per, 3) for k, v in c.items()}, "total": round(total / per, 3),
                     "dpp": round(dpp / per, 3)},
        "region": {**c, "total": total, "dpp": dpp},
    }


def mean(items):
    keys = items[0]["per_step"].keys()
    return {k: round(sum(i["per_step"][k] for i in items) / len(items), 3) for k in keys}


def analyse(text: str, kw: int):
    ins, branches = parse(text)
    index = {addr: i for i, (addr, _, _) in enumerate(ins)}
    found = {"alpha": [], "beta": [], "fold": [], "fold_generic": [], "fold_peeled": []}
    bodies = []   # fold bodies: (index of the first instruction, region)
    for reg in regions(ins, branches):
        f = features(reg)
        if f["rows"] == kw and f["nt_store"] >= kw:
            found["alpha"].append(reg)
        elif f["rows"] == kw and f["gstore"] == 0 and f["w64"] >= kw:
            found["beta"].append(reg)
        elif f["rows"] == 14 and f["b128"] >= 8 and f["w64"] == 0:
            bodies.append((index[reg[0][0]], reg))
    for n, (i0, reg) in enumerate(bodies):
        end = bodies[n + 1][0] if n + 1 < len(bodies) else min(len(ins), i0 + 2 * len(reg))
        back = [(i, branches[ins[i][0]]) for i in range(i0, end)
                if ins[i][0] in branches and branches[ins[i][0]] <= reg[0][0]]
        if not back:
            found["fold_peeled"].append(reg)
            continue
        loop = ins[index[min(t for _, t in back)]:max(i for i, _ in back) + 1]
        found["fold" if features(loop)["gstore"] <= 2 else "fold_generic"].append(loop)
    res = {"kernel_instructions": len(ins), "kw": kw}
    for name, regs in found.items():
        if not regs and name.startswith("fold_"):
            continue
        if not regs:
            sys.exit(f"no {name} region found: the anchoring no longer fits this build (see the docstring)")
        items = [count(r, kw) for r in regs]
        res[name] = {"instances": items, "per_step": mean(items)}
    return res, found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lib", nargs="?", default=os.path.join(REPO, "turbo_decoder_cuda_amd", "libturbo_mi355x.so"))
    ap.add_argument("--kernel", default=KERNEL)
    ap.add_argument("--kw", type=int, default=15)
    ap.add_argument("--json", help="write the counts here")
    ap.add_argument("--dump", help="write each region's instructions to DIR/<name><n>.s (for reading)")
    a = ap.parse_args()
    res, found = analyse(disassemble(a.lib, a.kernel), a.kw)
    res["kernel"] = a.kernel
    for name in ("alpha", "beta", "fold"):
        p = res[name]["per_step"]
        print(f"{name:5s} x{len(res[name]['instances'])}  per step: total {p['total']:7.2f}  " +
              "  ".join(f"{k} {p[k]:6.2f}" for k in CLASSES) + f"  (dpp {p['dpp']:.2f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for name, regs in found.items():
            for n, reg in enumerate(regs):
                with open(os.path.join(a.dump, f"{name}{n}.s"), "w") as f:
                    f.writelines(f"{addr:#x}\t{mn} {ops}\n" for addr, mn, ops in reg)


if __name__ == "__main__":
    main()
