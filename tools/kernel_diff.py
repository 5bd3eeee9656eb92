"""Are the kernels of two sets of .hip files instruction-identical?  For a refactor that moves kernels between files.
usage: kernel_diff.py OLD.hip[,OLD2.hip...] NEW.hip[,NEW2.hip...]   (run anywhere: cross-compiles the device side for gfx950, needs no GPU)
Each file's device side is compiled alone with the CXXFLAGS read from csrc/Makefile, disassembled, split per mangled kernel name; per kernel the instruction
text (the pc-relative distance to a __constant__ table masked) and the resource usage (-Rpass-analysis=kernel-resource-usage: SGPRs, VGPRs,
scratch, occupancy, LDS) are compared.  Exit status 1 if a kernel present on both sides differs or one is defined twice; kernels on one side
only are listed."""
import os, re, subprocess, sys, tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OBJDUMP = os.environ.get("OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
MAKEFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metafem.jl_amd", "csrc", "Makefile")
mk = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", open(MAKEFILE).read(), re.M))  # the library's own flags: CXXFLAGS with $(ARCH) filled in
FLAGS = mk["CXXFLAGS"].replace("$(ARCH)", os.environ.get("ARCH", mk["ARCH"])).split()


def kernels(path, out):
    """mangled name -> (instruction text, resource-usage lines) of the kernels defined in `path`, added to `out`"""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "dev.o")
        cc = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage", "-c",
                             os.path.abspath(path), "-o", obj], cwd=os.path.dirname(os.path.abspath(path)), capture_output=True, text=True, check=True)
        asm = subprocess.run([OBJDUMP, "-d", "--no-leading-addr", "--no-show-raw-insn", obj], capture_output=True, text=True, check=True).stdout
    usage, name = {}, None
    for line in cc.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+(\S.*?)\s*\[-Rpass-analysis)", line)
        if m and m.group(1):
            name = m.group(1)
        elif m and name:
            usage.setdefault(name, []).append(m.group(2))
    name = None
    text = {}
    for line in asm.splitlines():
        m = re.match(r"<(\S+)>:$", line)
        if m:
            name = m.group(1)
        elif name and line.strip():
            ins, prev = re.sub(r"\s*//.*$", "", line).strip(), text.setdefault(name, [])
            if ins.startswith("s_add") and any(q.startswith("s_getpc_b64") for q in prev[-2:]):
                ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)  # the distance to a __constant__ table: moves with the kernel's place in its file
            prev.append(ins)
    dup = 0
    for k, v in text.items():
        while v and v[-1] in ("s_nop 0", "s_code_end", "..."):  # alignment padding behind the kernel's last instruction (its length depends on what follows)
            v.pop()
        if k in out:
            print(f"DEFINED TWICE: {k}")
            dup = 1
        out[k] = ("\n".join(v), tuple(usage.get(k, ())))
    return dup


old, new, bad = {}, {}, 0
for p in sys.argv[1].split(","):
    bad |= kernels(p, old)
for p in sys.argv[2].split(","):
    bad |= kernels(p, new)
for k in sorted(set(old) | set(new)):
    if k not in new:
        print(f"removed    {k}")
    elif k not in old:
        print(f"added      {k}")
    else:
        same_text, same_use = old[k][0] == new[k][0], old[k][1] == new[k][1]
        bad |= not (same_text and same_use)
        print(f"{'identical ' if same_text and same_use else 'DIFFERENT '} {k}  ({len(old[k][0].splitlines())} instructions, "
              f"text {'=' if same_text else '!='}, resources {'=' if same_use else '!='}: {'; '.join(new[k][1])})")
print(f"{len(old)} kernels before, {len(new)} after, {len(set(old) & set(new))} on both sides: {'DIFFERENCES' if bad else 'all identical'}")
sys.exit(1 if bad else 0)
