"""The rounding contract of a serial chain, read off its gfx950 instructions: a file is compiled as the Makefile compiles it
(-ffp-contract=on) and the one function named must hold no fused multiply-add in any form."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lsp-dsp-units_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def assert_separate_multiplies_and_adds(tmp_path, source, function):
    out = os.path.join(str(tmp_path), source + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-w",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(PKG, "include"),
                           "-S", "--offload-device-only", os.path.join(CSRC, source), "-o", out])
    bodies, cur = {}, None
    for l in open(out).read().split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur and (l.startswith(".Lfunc_end") or ".amdhsa_kernel" in l):
            cur = None
        elif cur:
            bodies[cur].append(l.strip())
    names = [n for n in bodies if function in n]
    assert len(names) == 1, sorted(bodies)
    ops = [l.split()[0] for l in bodies[names[0]] if l and not l.startswith((";", "."))]
    assert len(ops) > 20
    fused = [o for o in ops if o.startswith(("v_fma", "v_fmac", "v_mad_f", "v_mac_f"))]
    assert not fused, fused
