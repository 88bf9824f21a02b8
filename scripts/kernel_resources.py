"""Register / scratch use of the kernels in a hipcc object (its gfx950 code object's metadata notes).

    python scripts/kernel_resources.py stochastic-epidemic-modelling_amd/lib/epipf_group.o [name-filter]
    python scripts/kernel_resources.py --digest stochastic-epidemic-modelling_amd/lib/epipf_incidence.o [name-filter]

--digest adds to each line the sha256 (first 16 hex digits) of the kernel's disassembly -- its instructions in order,
without addresses and encodings -- so that two builds can be compared kernel by kernel: equal digests are equal code.
Names are printed demangled when the tool chain's llvm-cxxfilt is there."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(obj, d):
    """Path of the object's gfx950 code object, extracted beside it; the caller removes what cleanup() lists."""
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", obj], cwd=d, capture_output=True, check=True)
    cos = [f for f in os.listdir(os.path.dirname(obj)) if f.startswith(os.path.basename(obj) + ".0.hipv4")]
    return os.path.join(os.path.dirname(obj), cos[0])


def cleanup(obj):
    for f in os.listdir(os.path.dirname(obj)):
        if f.startswith(os.path.basename(obj) + ".0.hipv4") or f.startswith(os.path.basename(obj) + ".0.host"):
            os.remove(os.path.join(os.path.dirname(obj), f))


def demangle(names):
    try:
        out = subprocess.run([f"{LLVM}/llvm-cxxfilt"] + names, capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def digests(co):
    """{symbol: digest} of every function in the code object's text."""
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                         capture_output=True, text=True, check=True).stdout
    out, name, h, pc = {}, None, None, 0
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line)
        if m:
            if name:
                out[name] = h.hexdigest()[:16]
            name, h, pc = m.group(1), hashlib.sha256(), 0
        elif name and line.strip():
            line = re.sub(r"\s*//.*$", "", line).strip()
            # a call's target is s_getpc_b64 plus a literal: the distance to the callee, which moves with the layout of
            # the code object (kernels added before it) while the code stays the same; so does the kernel's index among
            # the module's kernels, which a call hands to a callee that uses LDS (the implicit argument in s15)
            if pc > 0 and re.match(r"s_addc?_u32 ", line):
                line = re.sub(r"0x[0-9a-f]+$|-?\d+$", "PCREL", line)
            if re.match(r"s_mov_b32 s15, \d+$", line):
                line = "s_mov_b32 s15, KERNEL_ID"
            pc = 2 if line.startswith("s_getpc_b64") else pc - 1
            h.update((re.sub(r"<[^>+]+(\+0x[0-9a-f]+)?>", r"<\1>", line) + "\n").encode())   # branch targets: offsets only
    if name:
        out[name] = h.hexdigest()[:16]
    return out


def main():
    args = sys.argv[1:]
    want_digest = "--digest" in args
    args = [a for a in args if a != "--digest"]
    obj = os.path.abspath(args[0])
    filt = args[1] if len(args) > 1 else ""
    with tempfile.TemporaryDirectory() as d:
        try:
            co = code_object(obj, d)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            dig = digests(co) if want_digest else {}
        finally:
            cleanup(obj)
    keys = ["private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count",
            "group_segment_fixed_size"]
    short = {"private_segment_fixed_size": "scratch", "group_segment_fixed_size": "static_lds"}
    rows = []
    for blk in notes.split("  - .")[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m:
            continue
        vals = {k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "?"])[1] for k in keys}
        rows.append((m.group(1), vals))
    pretty = demangle([n for n, _ in rows])
    for name, vals in rows:
        if filt not in name and filt not in pretty[name]:
            continue
        line = " ".join(f"{short.get(k, k.replace('_count', ''))}={v}" for k, v in vals.items())
        if want_digest:
            line += f" digest={dig.get(name, '?')}"
        print(pretty[name], line)


if __name__ == "__main__":
    main()
