#!/usr/bin/env python3
"""Price a kernel's hot loop in SIMD-cycles from its disassembly, by instruction class, without a GPU.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --offload-device-only -S -o kernels.s csrc/epipf_kernels.hip
    python3 scripts/loop_cycles.py kernels.s --kernel 'pf_step_kernelILi0ELi1ELi0ELi64E'

Reads compiler assembly (`-S`) or `llvm-objdump -d` text.  The hot loop is the innermost loop (a label and a later
branch back to it) of the chosen kernel that holds the SSA event's marks: `v_log_f32`, `v_rcp_f32` and at least ten
`v_mad_u64_u32` (Philox4x32-10); `--all` prices the whole text instead (a snippet of the loop alone); `--main-path`
leaves out the blocks a wave skips when none of its lanes needs them (the f64 channel, the small-x logs).  Every VALU
instruction is put in a class and the class is priced in cycles per wave64 instruction per SIMD from the measured
tables: profiles/r1_isa_throughput.txt and profiles/isa_forms.txt (scripts/isa_forms.hip), or `--prices FILE` (JSON:
class or mnemonic -> cycles, e.g. profiles/isa_forms_prices.json).  Scalar, branch, wait and memory instructions are counted, not priced: they issue beside the VALU.
A tally of instruction classes: it says where the issue cycles of a loop go, not how long the kernel runs."""
import argparse
import json
import re
import sys

# cycles per wave64 instruction per SIMD.  r1: profiles/r1_isa_throughput.txt (ILP = 8 rows); forms: profiles/isa_forms.txt
PRICES = {
    "philox_product": 4.6,      # r1 k_mad_u64 4.59; v_mul_hi_u32 / v_mul_lo_u32 4.2-4.3
    "bitwise": 2.3,             # r1 k_xor 2.29, k_add_u32 2.27
    "arith": 4.2,               # r1 f32/f64 fma, mul, add, converts 3.9-4.3
    "packed_f32": 4.2,          # r1 k_pk_fma_f32 4.24: two f32 operations per instruction
    "compare": 6.6,             # into an SGPR pair or vcc: priced as r1's select until profiles/isa_forms.txt says otherwise
    "compare_f64": 8.5,         # r1 k_cmp_f64 8.52
    "select": 6.6,              # r1 k_cndmask 6.61 (SGPR-pair mask)
    "transcendental": 8.1,      # r1 k_log_f32 8.09, k_rcp_f32 8.32
    "transcendental_f64": 16.3,  # r1 k_rcp_f64
}
UNPRICED = ("scalar", "branch", "wait", "memory", "other")

_BITWISE = re.compile(
    r"v_(xor|and|or|not|xnor|bitop3|lshl|lshr|ashr|lshlrev|lshrrev|ashrrev|bfi|bfe|perm|alignbit|alignbyte|mov|add_u32|sub_u32|"
    r"subrev_u32|add_co|sub_co|subrev_co|addc_co|subb_co|add3|and_or|or3|xad|lshl_add|lshl_or|add_lshl|mbcnt|readlane|"
    r"readfirstlane|writelane|accvgpr|swap|min_u32|max_u32|min_i32|max_i32|add_i32|sub_i32)(_|$)")


def classify(m):
    """The class of mnemonic m (without its _e32 / _e64 / _dpp / _sdwa suffix)."""
    if m.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if m.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep", "s_setprio")):
        return "wait"
    if m.startswith("s_"):
        return "scalar"
    if m.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_")):
        return "memory"
    if not m.startswith("v_"):
        return "other"
    if m.startswith(("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_hi_u32", "v_mul_lo_u32", "v_mul_hi_i32", "v_mul_u32_u24",
                     "v_mul_hi_u32_u24", "v_mad_u32_u24")):
        return "philox_product"
    if m.startswith(("v_cmp_", "v_cmpx_")):
        return "compare_f64" if m.endswith("f64") else "compare"
    if m.startswith("v_cndmask"):
        return "select"
    if m.startswith(("v_rcp_", "v_log_", "v_exp_", "v_sqrt_", "v_rsq_", "v_sin_", "v_cos_")):
        return "transcendental_f64" if m.endswith("f64") else "transcendental"
    if m.startswith("v_pk_"):
        return "packed_f32"
    if _BITWISE.match(m):
        return "bitwise"
    return "arith"                                    # f32 / f64 mul, add, fma, converts, ldexp, frexp, min / max


_INST = re.compile(r"^\s*(?:[0-9a-fA-F]+:\s+)?([vs]_[a-z0-9_]+|global_[a-z0-9_]+|flat_[a-z0-9_]+|buffer_[a-z0-9_]+|"
                   r"scratch_[a-z0-9_]+|ds_[a-z0-9_]+)\b(.*)$")
_LABEL = re.compile(r"^([.\w$]+):")
_OBJ_LABEL = re.compile(r"^[0-9a-fA-F]+ <([.\w$]+)>:")
_SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")


def parse(text):
    """[(label or None, mnemonic or None, operands)] per line that is a label or an instruction."""
    out = []
    for line in text.splitlines():
        line = line.split(";")[0].split("//")[0].rstrip()
        if not line:
            continue
        lab = _OBJ_LABEL.match(line) or _LABEL.match(line)
        if lab:
            out.append((lab.group(1), None, ""))
            continue
        ins = _INST.match(line)
        if ins:
            out.append((None, _SUFFIX.sub("", ins.group(1)), ins.group(2)))
    return out


def kernel_slice(items, pattern):
    """The items of the first kernel whose label matches pattern, to its s_endpgm-terminated end (the next kernel)."""
    rx = re.compile(pattern)
    start = next((i for i, (lab, _, _) in enumerate(items) if lab and not lab.startswith(".") and rx.search(lab)), None)
    if start is None:
        raise SystemExit(f"no kernel matches {pattern!r}")
    end = next((i for i in range(start + 1, len(items)) if items[i][0] and not items[i][0].startswith(".")), len(items))
    return items[start:end]


def hot_loop(items):
    """The shortest loop (label .. backward branch to it) that holds the SSA event's marks."""
    at = {lab: i for i, (lab, _, _) in enumerate(items) if lab}
    best = None
    for i, (_, m, ops) in enumerate(items):
        if not m or not m.startswith(("s_cbranch", "s_branch")):
            continue
        tgt = ops.strip().split()[-1] if ops.strip() else ""
        tgt = tgt.strip("<>").split("+")[0]
        if tgt in at and at[tgt] < i:
            body = items[at[tgt]:i + 1]
            ms = [b[1] for b in body if b[1]]
            if (sum(x == "v_mad_u64_u32" for x in ms) >= 10 and any(x.startswith("v_log_f32") for x in ms)
                    and any(x.startswith("v_rcp_f32") for x in ms)):
                if best is None or len(body) < len(best):
                    best = body
    if best is None:
        raise SystemExit("no loop with the SSA event's marks (v_log_f32, v_rcp_f32, >= 10 v_mad_u64_u32)")
    return best


def main_path(items):
    """The items outside the loop's guarded blocks: what lies between an `s_cbranch_execz L` and a later label L of the
    same loop runs only for the lanes of a rare case (the f64 channel, the two small-x logs) and is skipped by a wave
    with no such lane."""
    at = {lab: i for i, (lab, _, _) in enumerate(items) if lab}
    keep = [True] * len(items)
    for i, (_, m, ops) in enumerate(items):
        if m == "s_cbranch_execz":
            tgt = ops.strip().split()[-1].strip("<>").split("+")[0] if ops.strip() else ""
            if tgt in at and at[tgt] > i:
                for k in range(i + 1, at[tgt]):
                    keep[k] = False
    return [it for it, k in zip(items, keep) if k]


def tally(items, prices):
    """{class: {"n", "cycles", "mnemonics": {m: n}}} and the totals."""
    table = {}
    for _, m, _ in items:
        if not m:
            continue
        c = classify(m)
        row = table.setdefault(c, {"n": 0, "cycles": 0.0, "mnemonics": {}})
        row["n"] += 1
        row["cycles"] += prices.get(m, prices.get(c, 0.0))             # a mnemonic's own price before its class's
        row["mnemonics"][m] = row["mnemonics"].get(m, 0) + 1
    valu = sum(r["n"] for c, r in table.items() if c not in UNPRICED)
    cycles = sum(r["cycles"] for c, r in table.items() if c not in UNPRICED)
    return {"classes": table, "valu": valu, "cycles": round(cycles, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="assembly (-S) or llvm-objdump -d text; - for stdin")
    ap.add_argument("--kernel", default="pf_step_kernelILi0ELi1ELi0ELi64E", help="regex on the kernel's symbol")
    ap.add_argument("--all", action="store_true", help="price every instruction of the text (a loop snippet)")
    ap.add_argument("--main-path", action="store_true", help="leave out the loop's guarded (rare-case) blocks")
    ap.add_argument("--prices", help="JSON file: class or mnemonic -> cycles, replacing the built-in entries it names")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    a = ap.parse_args(argv)
    text = sys.stdin.read() if a.asm == "-" else open(a.asm).read()
    prices = dict(PRICES)
    if a.prices:
        prices.update(json.load(open(a.prices)))
    items = parse(text)
    body = items if a.all else hot_loop(kernel_slice(items, a.kernel))
    if a.main_path:
        body = main_path(body)
    t = tally(body, prices)
    if a.json:
        print(json.dumps(t, sort_keys=True))
        return 0
    print(f"{'class':<20}{'n':>5}{'cyc each':>10}{'cycles':>9}  mnemonics")
    for c, r in sorted(t["classes"].items(), key=lambda kv: -kv[1]["cycles"]):
        ms = ", ".join(f"{m} x{n}" if n > 1 else m for m, n in sorted(r["mnemonics"].items(), key=lambda kv: -kv[1]))
        each = f"{prices[c]:.1f}" if c in prices and c not in UNPRICED else "-"
        print(f"{c:<20}{r['n']:>5}{each:>10}{r['cycles']:>9.1f}  {ms}")
    print(f"{'VALU':<20}{t['valu']:>5}{'':>10}{t['cycles']:>9.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
