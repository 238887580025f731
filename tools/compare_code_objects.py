"""Compare the gfx950 kernels of two builds, unit by unit.

    python tools/compare_code_objects.py BUILD_A BUILD_B PREFIX

BUILD_A, BUILD_B: directories of objects made by mdp_playground_amd/build.py; PREFIX: the units compared are PREFIX*.o.
Per unit the code object is unbundled (as tests/test_kernel_spills.py does) and three things are compared: the set of
kernel symbols, each kernel's metadata (register and spill counts, group and private segment sizes, kernarg size) and
each kernel's disassembly.  Prints the kernels that differ and the counts; exit status 1 if any does.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
KEYS = ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels(obj, tmp):
    """{kernel symbol: (metadata tuple, disassembly text)} of obj's gfx950 code object"""
    base = os.path.join(tmp, os.path.basename(obj))
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin")
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + base + ".fatbin", "--targets=" + TARGET,
        "--output=" + base + ".elf")
    meta = {}
    for block in re.split(r"\n  - ", run(f"{LLVM}/llvm-readelf", "--notes", base + ".elf"))[1:]:
        kv = dict(re.findall(r"^ {2,4}\.([a-z_]+):\s+(\S+)\s*$", "  " + block, re.M))      # (kernel-level keys only)
        if "symbol" in kv:
            meta[kv["name"]] = tuple(kv.get(k) for k in KEYS)
    # (a kernel reaches a constant table by s_getpc_b64 + a displacement, which moves with the kernel's place in the code
    #  object: the displacement is replaced by the symbol it lands in, and the addresses are dropped)
    syms = sorted((int(m.group(1), 16), m.group(2)) for m in re.finditer(r"^([0-9a-f]{16}) .{7} \S+\s+[0-9a-f]{16} (\S+)$", run(f"{LLVM}/llvm-objdump", "-t", base + ".elf"), re.M))
    text = {}
    for part in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", base + ".elf")):
        m = re.match(r"[0-9a-f]+ <([^>]+)>:\n", part)
        if not m:
            continue
        lines, pc = [], None
        for line in part[m.end():].splitlines():
            ins, _, addr = line.partition("//")
            ins = ins.rstrip()
            lit = re.search(r"^\ts_add_u32 (s\d+), \1, (0x[0-9a-f]+)$", ins) if pc is not None else None
            if lit:
                at = (pc + int(lit.group(2), 16)) & 0xFFFFFFFF      # (the low word; the tables lie within 4 GiB)
                sym = max((x for x in syms if x[0] & 0xFFFFFFFF <= at), default=(at, "?"))
                ins = ins[:lit.start(2)] + "%s+%d" % (sym[1], at - (sym[0] & 0xFFFFFFFF))
            pc = int(addr.split(":")[0], 16) + 4 if "s_getpc_b64" in ins else None if lit else pc
            lines.append(ins)
        text[m.group(1)] = "\n".join(lines)
    return {k: (meta[k], text.get(k)) for k in meta}


def main(dir_a, dir_b, prefix):
    units = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, prefix + "*.o"))})
    compared, differ = 0, []
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for u in units:
            a, b = (kernels(os.path.join(d, u), t) if os.path.exists(os.path.join(d, u)) else {} for d, t in ((dir_a, ta), (dir_b, tb)))
            for k in sorted(set(a) | set(b)):
                compared += 1
                what = [w for w, x in (("symbol", k not in a or k not in b), ("metadata", a.get(k, (0, 0))[0] != b.get(k, (0, 0))[0]),
                                       ("text", a.get(k, (0, 0))[1] != b.get(k, (0, 0))[1])) if x]
                if what:
                    differ.append(f"{u}: {k}: {', '.join(what)}")
    print("\n".join(differ))
    print(f"{len(units)} units, {compared} kernels compared, {len(differ)} differ")
    return 1 if differ or not compared else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
