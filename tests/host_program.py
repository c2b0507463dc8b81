"""The stand-alone host programs of the suite (tests/<name>_args_main.cpp): each runs the header
logic of one group of kernels on the CPU, under sanitizers, against a second implementation of its
own.  One statement of how they are built and run.  The library is built with -ffp-contract=off
(_lib.HIPCC_FLAGS), so these are too: a host compiler that contracts by default would compare
arithmetic the device never performs.  Nothing sanitised is loaded into the interpreter."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raynet_amd", "csrc")
ASAN_UBSAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run_host_program(name, tmp_path, sanitizers=ASAN_UBSAN, extra=()):
    """Builds tests/<name>_args_main.cpp into tmp_path and runs it: exit status 0 and
    '<name>_args: ok' at the end of what it printed -> that output."""
    exe = os.path.join(str(tmp_path), name + "_args")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall",
                           "-Werror", "-ffp-contract=off", *extra, *sanitizers, "-I", CSRC,
                           os.path.join(REPO, "tests", name + "_args_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith(name + "_args: ok"), r.stdout
    return r.stdout
