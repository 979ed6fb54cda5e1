"""Check that a host-only change left the device code alone: compile units of two csrc trees to gfx950 assembly (the Makefile's
CXXFLAGS plus --cuda-device-only -S), drop .file / .ident, source-path lines and comment-only lines, take the function's position
in its unit out of the local labels (.LBB<position>_<block>: it moves with the order of instantiation), and compare kernel by
kernel: every .amdhsa_kernel symbol present under the same name on both sides, instruction stream and kernel descriptor
identical.  "The same name" is the demangled one (c++filt) without its namespace qualifiers: a kernel's argument struct that moves
from the unit's anonymous namespace into a header both halves of the unit include changes the mangled symbol and nothing else.
Two kernels of a unit that reduce to one such name are an error.  The other tree needs ../../include/gpt_hip.h next to it, as in
a checkout.  The default list is the Makefile's SRCS without its ONESHOT_HOST: the *_host.hip halves of the one-shot units hold no
kernel.
usage: python tools/device_isa_diff.py OTHER_CSRC [unit.hip ...]   (CPU only; hipcc cross-compiles; exit 1 on any difference)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-value", "-fno-gpu-rdc", "--cuda-device-only", "-S"]


def kernels(csrc, unit, out):
    """{kernel symbol: (instruction stream, descriptor)} of one unit, normalised."""
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(csrc, unit), "-o", out], check=True, stderr=subprocess.DEVNULL)
    lines = [x.rstrip() for x in open(out)]
    lines = [x for x in lines if x.strip() and not x.lstrip().startswith((";", "//", ".file", ".ident")) and csrc not in x]
    s = "\n".join(re.sub(r"\s*;.*$", "", x) for x in lines)
    s = re.sub(r"\.L(BB|JTI|CPI)\d+_", r".L\1_", s)
    found = {}
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", s, flags=re.M)
    if not shutil.which("c++filt"):
        sys.exit("device_isa_diff: c++filt (binutils) is needed to compare kernels by their demangled names")
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    for name, demangled in zip(names, plain):
        key = re.sub(r"\(anonymous namespace\)::|\bgpt::", "", demangled)
        if key in found:                   # two kernels of a unit under one key: one would drop out of the comparison unseen
            sys.exit(f"device_isa_diff: {unit}: two kernels reduce to the name {key}")
        i = s.index("\n" + name + ":\n")
        body = s[i:s.index(".Lfunc_end", i)]
        j = s.index(".amdhsa_kernel " + name + "\n")
        found[key] = (body.replace(name, key), s[j:s.index(".end_amdhsa_kernel", j)].replace(name, key))
    assert len(found) == len(names), (unit, len(found), len(names))
    return found


def makefile_list(name):
    """The words of the Makefile variable `name` (continuation lines joined), without references to other variables."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    value = re.search(rf"^{name}\s*=(.*)$", text, flags=re.M).group(1)
    return [w for w in value.split() if not w.startswith("$(")]


def main():
    other = os.path.abspath(sys.argv[1])
    host_halves = set(makefile_list("ONESHOT_HOST"))
    units = sys.argv[2:] or [u for u in makefile_list("SRCS") if u not in host_halves]
    bad = 0
    for unit in [u for u in units if not os.path.exists(os.path.join(other, u))]:
        print(f"{unit}: not in {other} (a new unit): nothing to compare")
        units.remove(unit)
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(max_workers=os.cpu_count() or 1) as ex:
        jobs = {(side, unit): ex.submit(kernels, csrc, unit, os.path.join(d, f"{side}_{unit}.s"))
                for unit in units for side, csrc in (("a", other), ("b", CSRC))}
        for unit in units:
            a, b = jobs["a", unit].result(), jobs["b", unit].result()
            diff = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
            print(f"{unit}: {len(b)} kernels, " + ("identical" if not diff else "DIFFERENT: " + ", ".join(diff)))
            bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
