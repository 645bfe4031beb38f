"""What the CPU tests of the kernel units and of csrc/wbc_layout.h share: the compiler's resource report of a
one-kernel unit, and the build and run of a test's stand-alone host program.  A plain module: no test, no fixture."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadrupedwholebodycontroller_amd", "csrc")


def report(unit, var):
    """The compiler's resource report (-Rpass-analysis=kernel-resource-usage) of a one-kernel unit
    under its Makefile flags, {kernel: {field: value}}, and its device assembly."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    waves = re.search(r"^WAVES \?= (\d+)", mk, re.M).group(1)
    kflags = re.search(r"^KFLAGS := (.*)$", mk, re.M).group(1).split()
    sflags = re.search(rf"^{var} := (.*)$", mk, re.M).group(1).split()
    assert unit in re.search(r"^KTU := (.*)$", mk, re.M).group(1).split()
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, f"-DWBC_WAVES_PER_SIMD={waves}", *kflags, *sflags, "-S", "--offload-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, f"wbc_kernel_{unit}.hip"), "-o", "-"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(2).isdigit():
            cur[m.group(1)] = int(m.group(2))
    return out, r.stdout


def build_host_program(d, stem, prog):
    """`prog` as d/stem.cpp, built against include/ and csrc/ with the address and undefined-behaviour sanitizers
    when the host toolchain links them (a stand-alone program: nothing is preloaded), else without; its path."""
    src = d / f"{stem}.cpp"
    src.write_text(prog)
    exe = d / stem
    cmd = ["g++", "-O1", "-g", "-Wall", "-Wno-unused-result", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           str(src), "-o", str(exe)]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True)
    if san.returncode != 0 or subprocess.run([str(exe), "names"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return str(exe)


def run_host_program(exe, mode, text=""):
    """The program's `mode` on `text`: its output lines, split into fields."""
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l.split() for l in r.stdout.splitlines()]
