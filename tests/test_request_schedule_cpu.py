"""The block kernels' prologue waits with `s_waitcnt vmcnt(N)` for the input patch and the per-channel constants only, N =
the load instructions of the weight queue requested behind them (csrc/request_schedule.h). The formulas are constexpr
functions in a header without HIP types: a host program evaluates them here, for every (queue depth, element type) the
sources instantiate."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unina-yolo-dla_amd", "csrc")
VMCNT_MAX = 63                 # 6-bit field of s_waitcnt on gfx9
WBLK = {"EltH": 1024, "EltI8": 1024, "EltS": 2048}      # bytes per weight block (block_pipeline.h)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "request_schedule.h"
using namespace unina::sched;
static_assert(kVmcntMax == 63, "vmcnt field");
static_assert(loads_per_block(1024) == 1 && loads_per_block(2048) == 2, "loads per block");
static_assert(prologue_wait(16, 100, 1024) == 16 && prologue_wait(8, 100, 2048) == 16, "N = D x loads per block");
static_assert(prologue_wait(16, 5, 1024) == 5, "a sequence shorter than the queue");
static_assert(prologue_wait_fits(16, 100, 2048) && !prologue_wait_fits(32, 100, 2048), "fits");
int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    const int d = atoi(argv[i]), total = atoi(argv[i + 1]), wblk = atoi(argv[i + 2]);
    printf("%d %d %d %d %d\n", d, total, wblk, prologue_wait(d, total, wblk), (int)prologue_wait_fits(d, total, wblk));
  }
  return 0;
}
"""


def _args(text):
    return [a.strip() for a in text.split(",")]


def instantiated():
    """(D, element type) of every block / pair / tile-head instantiation named in the sources."""
    found = set()
    c3 = open(os.path.join(CSRC, "c3k2_fused.hip")).read()
    table = c3[c3.index("const Class kClasses[]"):]
    for macro, args in re.findall(r"^\s*(C3K2\w*)\(([^)]*)\)", table, re.M):
        elt = "EltS" if macro in ("C3K2X", "C3K2XS") else ("EltI8" if macro.startswith("C3K2I") else "EltH")
        found.add((int(_args(args)[6]), elt))
    srcs = "".join(open(os.path.join(CSRC, f)).read() for f in ("c3k2_fused.hip", "block_dual.hip", "conv_pair.hip", "head_fused.hip"))
    for args in re.findall(r"c3k2_fused_body<([0-9][^>]*)>", srcs) + re.findall(r"BLOCK_DUAL_WS\(\w+,\s*([0-9][^)]*)\)", srcs):
        a = _args(args)
        found.add((int(a[6]), a[8] if len(a) > 8 else "EltH"))
    for args in re.findall(r"conv_pair_kernel<([0-9][^>]*)>", srcs):
        a = _args(args)
        found.add((int(a[6]), a[8]))
    for args in re.findall(r"head_fused_(?:body|kernel)<([0-9][^>]*)>", srcs):
        found.add((int(_args(args)[4]), "EltH"))
    return sorted(found)


@pytest.fixture(scope="module")
def schedule(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched")
    src = d / "sched.cpp"
    src.write_text(PROGRAM)
    exe = d / "sched"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(triples):
        out = subprocess.run([str(exe)] + [str(v) for t in triples for v in t], capture_output=True, text=True, check=True).stdout
        return [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    return run


def test_sources_instantiate_the_expected_families():
    inst = instantiated()
    assert {e for _, e in inst} == {"EltH", "EltI8", "EltS"}, inst
    assert {d for d, _ in inst} == {4, 8, 16}, inst


def test_prologue_wait_is_depth_times_loads_per_block_and_fits(schedule):
    inst = instantiated()
    rows = schedule([(d, 1000, WBLK[e]) for d, e in inst])
    assert len(rows) == len(inst)
    for (d, e), (d2, _, wblk, n, fits) in zip(inst, rows):
        assert d2 == d and n == d * (wblk // 1024), (d, e, n)
        assert n <= VMCNT_MAX and fits == 1, (d, e, n)


def test_short_sequences_and_the_field_limit(schedule):
    rows = schedule([(16, 3, 1024), (16, 3, 2048), (63, 1000, 1024), (64, 1000, 1024), (32, 1000, 2048)])
    assert [r[3] for r in rows] == [3, 6, 63, 64, 64]
    assert [r[4] for r in rows] == [1, 1, 1, 0, 0]

