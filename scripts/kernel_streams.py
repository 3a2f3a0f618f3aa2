#!/usr/bin/env python3
"""Compare the device code of env_kernels.hip between a git revision and the
working tree, kernel by kernel (runs on a CPU box; hipcc cross-compiles).

    python scripts/kernel_streams.py --base HEAD [--must-match REGEX]

Both trees are compiled with the Makefile's HIPFLAGS plus --cuda-device-only -S
-Rpass-analysis=kernel-resource-usage.  Per kernel symbol the instruction
stream (directives and comments dropped, local labels renumbered) is reported
as `same` or `differs`, beside the VGPRs, SGPRs, scratch, LDS and occupancy of
both builds; symbols present on one side only are listed.  It compares streams
and resource figures, nothing else.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "drone_rl_amd/csrc"
FIGS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))
LABEL = re.compile(r"\.L[\w$.]+")


def split_kernels(asm):
    """{symbol: [instruction, ...]} of an AMDGPU assembly text."""
    out, cur = {}, None
    for line in asm.splitlines():
        line = re.split(r"\s;|^;", line, maxsplit=1)[0].strip()
        if not line:
            continue
        m = re.fullmatch(r"([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L"):
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".amdgpu_metadata"):
            break       # the YAML notes that follow hold no code
        elif line.startswith(".end_amdhsa_kernel") or line.startswith(".section"):
            cur = None
        elif cur is not None and not (line.startswith(".") and not LABEL.match(line)):
            cur.append(line)
    return {k: normalise(v) for k, v in out.items() if v}


def normalise(lines):
    """Renumber local labels in order of first appearance."""
    names = {}
    sub = lambda m: names.setdefault(m.group(0), ".L%d" % len(names))
    return [LABEL.sub(sub, " ".join(l.split())) for l in lines]


def parse_remarks(text):
    """{symbol: {figure: value}} of -Rpass-analysis=kernel-resource-usage."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        for label, key in FIGS:
            m = re.search(r"remark: .*\s" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def compare(base, new, res_base=None, res_new=None, must_match=None, out=sys.stdout):
    """Print the per-kernel report; the number of --must-match violations."""
    res_base, res_new, bad = res_base or {}, res_new or {}, 0
    fig = lambda r: " ".join("%s=%s" % (k, r.get(k, "?")) for _, k in FIGS)
    must = re.compile(must_match) if must_match else None
    for name in sorted(set(base) | set(new)):
        if name not in base or name not in new:
            verdict = "missing in %s" % ("base" if name not in base else "new")
        elif base[name] == new[name] and res_base.get(name) == res_new.get(name):
            verdict = "same"
        else:
            verdict = "differs (%d -> %d instructions)" % (len(base[name]), len(new[name]))
        print("%s: %s\n    base %s\n    new  %s" % (name, verdict, fig(res_base.get(name, {})),
                                                  fig(res_new.get(name, {}))), file=out)
        if must and must.search(name) and verdict != "same":
            bad += 1
    return bad


def hipflags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", os.environ.get("ARCH", "gfx950")).split()


def build(csrc):
    """(assembly, remarks) of env_kernels.hip under `csrc`."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + hipflags(csrc) + ["--cuda-device-only", "-S",
                                     "-Rpass-analysis=kernel-resource-usage",
                                     "env_kernels.hip", "-o", "-"]
    p = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr)
    return p.stdout, p.stderr


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--base", default="HEAD", help="git revision to compare against")
    ap.add_argument("--must-match", metavar="REGEX",
                    help="exit non-zero if a kernel matching it differs or is missing")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC, "include"],
                             check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        asm_b, rem_b = build(os.path.join(tmp, CSRC))
    asm_n, rem_n = build(os.path.join(ROOT, CSRC))
    base, new = split_kernels(asm_b), split_kernels(asm_n)
    bad = compare(base, new, parse_remarks(rem_b), parse_remarks(rem_n), a.must_match)
    same = sum(1 for k in base if new.get(k) == base[k])
    print("%d kernels in base, %d in new, %d with the same stream" % (len(base), len(new), same))
    if bad:
        print("%d kernel(s) matching %r differ or are missing" % (bad, a.must_match))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
