"""The stand-alone host programs of the CPU tests (tests/*_host.cpp: a csrc header compiled by g++, no HIP, no GPU), each built
twice -- plain, and under -fsanitize=undefined,address -- and run as a pair; and the checks that include/unina_mi355.h is plain C99."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
C99 = ["-std=c99", "-Wall", "-Wpedantic", "-Werror"]


def build_pair(tmp_dir, src):
    """tests/`src` -> [plain executable, sanitised executable] in tmp_dir."""
    cxx = shutil.which("g++")
    assert cxx, f"g++ is needed to build tests/{src}"
    exes = []
    for name, extra in (("plain", []), ("san", ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"])):
        exe = str(tmp_dir / name)
        subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", src), "-o", exe], check=True,
                       cwd=ROOT)
        exes.append(exe)
    return exes


def run_pair(exes, tmp_dir, payload, dtype=np.int32, canon=None, stdout=False):
    """Both builds on one input: `payload` is written to a case file and each build run as `exe case.in case.out`; the sanitised
    build must exit 0 and give the plain build's bytes. Returns the one output as a `dtype` array (with stdout=True: the array
    and what the programs printed, which must agree as well). dtype=None: the program writes no file. payload=None: the program
    takes no arguments at all. canon(array) is applied to each build's output before the two are compared."""
    src, dst = str(tmp_dir / "case.in"), str(tmp_dir / "case.out")
    if payload is not None:
        with open(src, "wb") as f:
            f.write(payload)
    got = []
    for exe in exes:
        if os.path.exists(dst):
            os.remove(dst)
        r = subprocess.run([exe] if payload is None else [exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        out = None if payload is None or dtype is None else np.fromfile(dst, dtype=dtype)
        got.append((out if canon is None or out is None else canon(out), r.stdout))
    (a, said_a), (b, said_b) = got
    assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert said_a == said_b
    return (a, said_a) if stdout else a


def assert_header_is_c99():
    """gcc -std=c99 -Wpedantic -Werror on the public header itself, without the HIP headers."""
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", *C99, "-DUNINA_NO_HIP_HEADERS", os.path.join(INCLUDE, "unina_mi355.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def compile_c99(tmp_path, body):
    """A C translation unit of `body` behind the public header (and <stddef.h>), compiled with -Wpedantic -Werror."""
    src = tmp_path / "unit.c"
    src.write_text('#define UNINA_NO_HIP_HEADERS\n#include "unina_mi355.h"\n#include <stddef.h>\n' + body)
    r = subprocess.run(["gcc", *C99, "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "unit.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
