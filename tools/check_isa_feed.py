"""Compile csrc/gpt_predict_i8.hip (device code) to assembly as tools/check_isa_spills.py does and report, per k_var_i8
instantiation, how the straight-line full tile (the basic block of 256 MFMAs) is fed:
  * per step of 32 MFMAs, the operands of the s_waitcnt instructions between the step's first and last MFMA, in order, each with
    the number of the step's MFMAs issued before it (a wait carrying lgkmcnt(0) there means an LDS read is awaited with nothing
    else outstanding: no lookahead), and the waits in front of the step;
  * for every A-fragment load (a global_load whose destination an MFMA reads as its A operand), the number of MFMAs between the
    load and the first MFMA that reads it — the block is a loop body, so the count runs on from its end into its beginning;
  * the scratch (spill) instructions in the blocks that hold MFMAs, which must be 0.
Exit status 1 if a wait inside a step other than the step's last carries lgkmcnt(0), if an A load has fewer than MIN_COVER MFMAs
to its first use, or if an MFMA block holds a scratch instruction.
usage: python tools/check_isa_feed.py [--min-cover N] [-DFLAG ...]   (CPU only; hipcc cross-compiles)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc", "gpt_predict_i8.hip")
args = sys.argv[1:]
MIN_COVER = 64
if "--min-cover" in args:
    i = args.index("--min-cover")
    MIN_COVER = int(args[i + 1])
    del args[i:i + 2]
with tempfile.TemporaryDirectory() as d:
    out = os.path.join(d, "dev.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-value", "-fno-gpu-rdc",
                        "--cuda-device-only", "-S", SRC, "-o", out] + args, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if r.returncode != 0:
        sys.exit("hipcc failed")
    s = open(out).read()


def basic_blocks(body):
    blocks, cur = [], []
    for line in body.split("\n"):
        if line.startswith(".LBB"):
            blocks.append(cur); cur = []
        cur.append(line)
    blocks.append(cur)
    return blocks


def regs(op):
    """the registers an operand like v[8:11] or v7 names"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", op)
    return {int(m.group(1))} if m else set()


def operands(line):
    return [x.strip() for x in line.split(None, 1)[1].split(",")] if len(line.split(None, 1)) > 1 else []


bad = 0
for name in re.findall(r"^(_ZN3gpt8k_var_i8I\w+):", s, flags=re.M):
    i = s.index("\n" + name + ":")
    body = s[i:s.index(".end_amdhsa_kernel", i)]
    kt = re.search(r"k_var_i8ILi(\d)", name).group(1)
    hot = [b for b in basic_blocks(body) if any("v_mfma_i32" in x for x in b)]
    spilled = sum("scratch_" in x for b in hot for x in b)
    full = [b for b in hot if sum("v_mfma_i32" in x for x in b) == 256]
    print(f"k_var_i8<KT={kt}>: {len(hot)} blocks hold MFMAs, scratch operations in them: {spilled}; blocks of 256 MFMAs: {len(full)}")
    if spilled or len(full) != 1:
        bad += 1
    if len(full) != 1:
        continue
    ins = [x.strip() for x in full[0] if x.startswith("\t") and not x.strip().startswith(";")]
    mf = [k for k, x in enumerate(ins) if x.startswith("v_mfma_i32")]
    # waits per step
    for st in range(8):
        first, last = mf[32 * st], mf[32 * st + 31]
        prev = mf[32 * st - 1] if st else -1
        before = [x.split(None, 1)[1] for x in ins[prev + 1:first] if x.startswith("s_waitcnt")]
        inside = []
        for k in range(first, last):
            if ins[k].startswith("s_waitcnt"):
                inside.append((sum(1 for q in mf[32 * st:32 * st + 32] if q < k), ins[k].split(None, 1)[1]))
        loads = sum(x.startswith("global_load") for x in ins[prev + 1:last])
        reads = sum(x.startswith("ds_read") for x in ins[prev + 1:last])
        print(f"  step {st}: {loads} global_load, {reads} ds_read; waits in front: {' | '.join(before) or '-'}")
        print("    inside (MFMAs of the step issued before the wait): " + "  ".join(f"{n}:{w}" for n, w in inside))
        for n, w in inside:
            if "lgkmcnt(0)" in w and n < 28:
                print(f"    ! lgkmcnt(0) after {n} MFMAs of step {st}")
                bad += 1
    # MFMA distance from each A load to its first use
    covers = []
    for k, x in enumerate(ins):
        if not x.startswith("global_load_dwordx4"):
            continue
        dst = regs(operands(x)[0])
        order = list(range(k + 1, len(ins))) + list(range(0, k))
        n, found = 0, None
        for q in order:
            y = ins[q]
            if y.startswith("v_mfma_i32"):
                ops = operands(y)
                if regs(ops[1]) & dst:
                    found = n
                    break
                n += 1
            elif y.startswith(("global_load", "ds_read", "v_")) and operands(y) and regs(operands(y)[0]) & dst:
                break               # overwritten (or read by something else first: a chunk piece on its way to LDS)
            elif y.startswith("ds_write") and any(regs(o) & dst for o in operands(y)):
                break
        if found is not None:
            covers.append(found)
    print(f"  A loads: {len(covers)}, MFMAs from the load to the first MFMA that reads it: min {min(covers) if covers else '-'}, "
          f"max {max(covers) if covers else '-'}")
    if not covers or min(covers) < MIN_COVER:
        bad += 1
sys.exit(1 if bad else 0)
