#!/usr/bin/env python
"""Is the DEVICE code of two csrc/ trees the same?  (what a host-only refactor has to show)

    python tools/device_isa_diff.py A_CSRC B_CSRC [-DRN_EXACT_BP_MATH ...]

Compiles raynet_hip.hip of both trees to gfx950 assembly (the library's own flags, device side
only, no GPU needed; about a minute each, side by side) and compares, kernel by kernel, the
instruction text and the .amdhsa_kernel descriptor (VGPRs, SGPRs, LDS, scratch).  Two things
differ between any two sources and are replaced first: the __hip_cuid_<hash> symbol (a hash of
the source text) and the function index in local labels (.LBB<k>_<n> and the comments that cite
them, .Lfunc_begin<k>, .Lfunc_end<k>: moving code between files renumbers functions; the blanks
in front of a comment, which pad it to a column, go with them).  Prints
the kernel count and `identical` or the first kernel that differs; the exit status is non-zero on a difference.
Kernels only B has (a feature's new ones) are listed and are no difference; a kernel only A has is one.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VOLATILE = [(re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_X"),
            (re.compile(r"(?:(?<=\.L)|\b)BB\d+_"), "BBk_"),      # .LBB<k>_<n>, and BB<k>_<n> in loop comments
            (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1k"),
            # a label's trailing comment is padded to a column: one more digit in <k> moves it
            (re.compile(r"[ \t]+;"), " ;")]


def compile_isa(csrc, out, extra=()):
    from raynet_amd._lib import HIPCC_FLAGS
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + flags + list(extra) +
                          ["--cuda-device-only", "-S", "raynet_hip.hip", "-o", out],
                          cwd=os.path.abspath(csrc))
    return out


def kernels(path):
    """{kernel symbol: (instruction text, descriptor block)} of one assembly file"""
    text = open(path).read()
    for pat, repl in VOLATILE:
        text = pat.sub(repl, text)
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel$", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_endk:" % re.escape(name), text, re.M | re.S)
        if body is None:
            raise SystemExit("%s: no body for kernel %s" % (path, name))
        out[name] = (body.group(0), m.group(0))
    return out


def compare(a, b):
    """(kernel count of a, None) or (count, what differs first)"""
    if set(a) - set(b):
        only = sorted(set(a) - set(b))
        return len(a), "%d kernels of A are missing in B, e.g. %s" % (len(only), only[0])
    for name in sorted(a):
        for what, x, y in zip(("instructions", "descriptor"), a[name], b[name]):
            if x != y:
                lx, ly = x.splitlines(), y.splitlines()
                at = next((i for i, (p, q) in enumerate(zip(lx, ly)) if p != q), min(len(lx), len(ly)))
                return len(a), "%s of %s differ at line %d:\n  A: %s\n  B: %s" % (
                    what, name, at, lx[at] if at < len(lx) else "<end>", ly[at] if at < len(ly) else "<end>")
    return len(a), None


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    a_csrc, b_csrc, extra = argv[0], argv[1], argv[2:]
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(2) as pool:
            fa = pool.submit(compile_isa, a_csrc, os.path.join(tmp, "a.s"), extra)
            fb = pool.submit(compile_isa, b_csrc, os.path.join(tmp, "b.s"), extra)
            ka, kb = kernels(fa.result()), kernels(fb.result())
            count, diff = compare(ka, kb)
    label = " ".join(extra) or "default build"
    added = sorted(set(kb) - set(ka))
    if added:
        print("%s: %d kernels only in B: %s" % (label, len(added), " ".join(added)))
    if diff:
        print("%s: %d kernels, DIFFERENT: %s" % (label, count, diff))
        return 1
    print("%s: %d kernels, identical" % (label, count))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
