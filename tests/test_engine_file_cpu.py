"""The engine loader refuses every file that would send a kernel out of bounds, and keeps accepting every file the exporter
writes. unina_load_engine turns the tables of a .une file into kernel pointers, leading dimensions and offsets that the
kernels trust; csrc/engine_validate.h is the one place that checks them. Here its verdict is compared with a reference model
in Python integers (engine_file_cases.defect), on the exporter's own files, on a corpus of named defects and on every numeric
field of a file set to seven values.

No file this module damages is given to unina_load_engine, to Engine(...) or to anything that launches: the verdict comes from
a stand-alone program over the header (plain, and under -fsanitize=undefined,address) and from the host-only hook
unina_debug_fusable_groups, which runs in a child process."""
import os
import subprocess
import sys
import time

import pytest

import engine_file_cases as F
import hostprog

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib(pkg):
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    return engine.load_library()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return hostprog.build_pair(tmp_path_factory.mktemp("engine_validate_host"), "engine_validate_host.cpp")


def _export(pkg, sd, g, precision, amax=None):
    from unina_yolo_dla_amd import export
    p = F.PRECISIONS[precision]
    if p == export.INT8 and amax is None:
        amax = F.unit_ranges(sd, g)
    return export.EngineBuilder(sd, g, p, amax).tobytes()


@pytest.fixture(scope="module")
def bases(pkg, sd7):
    """The 64x64 files of the seed-7 weights the corpus and the sweep damage: fp16, STRICT, and int8 with the ranges of
    test_abi_cpu.py's recipe (two emulated frames)."""
    from unina_yolo_dla_amd import export
    from emulate import run_op_table
    g = pkg.graph.Graph(in_h=64, in_w=64)
    b16 = export.EngineBuilder(sd7, g)
    amax = export.calibrate(run_op_table(b16, pkg.rng.frame(5000 + i, 64, 64))[1] for i in range(2))
    return {"fp16": b16.tobytes(), "strict": _export(pkg, sd7, g, "strict"), "int8": _export(pkg, sd7, g, "int8", amax),
            "fp32": _export(pkg, sd7, g, "fp32")}


def _program(exes, tmp_path, base, cases):
    """{case id: code} from both builds of the stand-alone program (which must agree), and what they printed per case."""
    import numpy as np
    out, said = hostprog.run_pair(exes, tmp_path, F.pack_cases(base, cases), dtype=np.int32, stdout=True)
    rec = out.reshape(-1, 2)
    assert [int(i) for i in rec[:, 0]] == [cid for cid, _ in cases]
    return {int(i): int(c) for i, c in rec}, dict(ln.split(" ", 1) for ln in said.splitlines())


def _hook_child(tmp_path, base, cases, names=None):
    """{case id: (rc, message)} from unina_debug_fusable_groups in ONE child process over all `cases`."""
    payload, work = str(tmp_path / "hook_cases.bin"), str(tmp_path / "hook_work.une")
    with open(payload, "wb") as f:
        f.write(F.pack_cases(base, cases))
    # (the loader allocates and frees the 10 MB blob twice per file: kept on the child's heap they are not page-faulted in again per case)
    env = dict(os.environ, MALLOC_MMAP_THRESHOLD_=str(1 << 30), MALLOC_TRIM_THRESHOLD_=str(1 << 30), MALLOC_TOP_PAD_=str(1 << 26))
    r = subprocess.run([sys.executable, os.path.join(HERE, "engine_file_child.py"), payload, work], capture_output=True, text=True, env=env)
    got, begun = {}, None
    for ln in r.stdout.splitlines():
        part = ln.split(" ", 3)
        if part[0] == "BEGIN":
            begun = int(part[1])
        elif part[0] == "END":
            got[int(part[1])] = (int(part[2]), part[3] if len(part) > 3 else "")
            begun = None
    label = (names or {}).get(begun, begun)
    assert r.returncode == 0 and begun is None, f"the loader's host side died (exit {r.returncode}) on case {label}\n{r.stderr[-1500:]}"
    assert sorted(got) == sorted(cid for cid, _ in cases)
    return got


# ---- 1. accepted files stay accepted ----------------------------------------------------------------------------------------
def _geometries():
    import emulate as E
    out = [(f"{h}x{w}", dict(in_h=h, in_w=w)) for h, w in (*E.PER_OP_SIZES, (64, 64), (640, 640))]
    out += list(E.PER_OP_TOPOLOGIES)
    out.append(("lite_p2-64x64", dict(lite_p2=True, in_h=64, in_w=64)))
    return out


# Fusable groups the PARENT of the validator's commit found in each file (unina_debug_fusable_groups of that library on the same
# bytes): the validator moves checks, it must not change what the matchers see. 64x64: as test_abi_cpu.py asserts them.
# (B-32x96 joined emulate.PER_OP_TOPOLOGIES later: what the planner, unchanged since, finds in it -- the figures of B-32x32.)
GROUPS = {
    ("fp16", "16x16"): 9, ("fp16", "16x48"): 9,
    ("fp16", "80x112"): 9, ("fp16", "96x160"): 9,
    ("fp16", "64x64"): 9, ("fp16", "640x640"): 9,
    ("fp16", "B-32x32"): 9, ("fp16", "B-96x160"): 9,
    ("fp16", "B-32x96"): 9,
    ("fp16", "lite_p2"): 8, ("fp16", "base16"): 9,
    ("fp16", "classes1"): 9, ("fp16", "classes7"): 9,
    ("fp16", "classes20"): 8, ("fp16", "lite_p2-64x64"): 8,
    ("fp32", "16x16"): 0, ("fp32", "16x48"): 0,
    ("fp32", "80x112"): 0, ("fp32", "96x160"): 0,
    ("fp32", "64x64"): 0, ("fp32", "640x640"): 0,
    ("fp32", "B-32x32"): 0, ("fp32", "B-96x160"): 0,
    ("fp32", "B-32x96"): 0,
    ("fp32", "lite_p2"): 0, ("fp32", "base16"): 0,
    ("fp32", "classes1"): 0, ("fp32", "classes7"): 0,
    ("fp32", "classes20"): 0, ("fp32", "lite_p2-64x64"): 0,
    ("int8", "16x16"): 9, ("int8", "16x48"): 9,
    ("int8", "80x112"): 9, ("int8", "96x160"): 9,
    ("int8", "64x64"): 9, ("int8", "640x640"): 9,
    ("int8", "B-32x32"): 9, ("int8", "B-96x160"): 9,
    ("int8", "B-32x96"): 9,
    ("int8", "lite_p2"): 8, ("int8", "base16"): 9,
    ("int8", "classes1"): 9, ("int8", "classes7"): 9,
    ("int8", "classes20"): 8, ("int8", "lite_p2-64x64"): 8,
    ("strict", "16x16"): 8, ("strict", "16x48"): 8,
    ("strict", "80x112"): 8, ("strict", "96x160"): 8,
    ("strict", "64x64"): 8, ("strict", "640x640"): 8,
    ("strict", "B-32x32"): 7, ("strict", "B-96x160"): 7,
    ("strict", "B-32x96"): 7,
    ("strict", "lite_p2"): 7, ("strict", "base16"): 8,
    ("strict", "classes1"): 8, ("strict", "classes7"): 8,
    ("strict", "classes20"): 8, ("strict", "lite_p2-64x64"): 7,
}


@pytest.mark.parametrize("precision", sorted(F.PRECISIONS))
def test_exported_files_stay_accepted(pkg, sd7, lib, exes, bases, tmp_path, precision):
    for label, kw in _geometries():
        g = pkg.graph.Graph(**kw)
        default = kw == dict(in_h=g.in_h, in_w=g.in_w)
        sd = sd7 if default else pkg.synth.make_state_dict(7, g)
        raw = bases[precision] if (label, default) == ("64x64", True) else _export(pkg, sd, g, precision)
        assert F.defect(raw) is None, (precision, label, F.defect(raw))
        codes, _ = _program(exes, tmp_path, raw, [(0, [])])
        assert codes == {0: F.OK}, (precision, label)
        path = tmp_path / "a.une"
        path.write_bytes(raw)
        assert lib.unina_debug_fusable_groups(str(path).encode()) == GROUPS[precision, label], (precision, label, lib.unina_last_error(None))


# ---- 2. the corpus ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", F.ALL)
def test_corpus_is_refused_with_its_code(lib, exes, bases, tmp_path, base):
    lay = F.Layout(bases[base])
    names = sorted(n for n, c in F.CORPUS.items() if base in c[0])
    cases = [(i, F.CORPUS[n][1](lay)) for i, n in enumerate(names)]
    codes, said = _program(exes, tmp_path, lay.raw, cases)
    hook = _hook_child(tmp_path, lay.raw, cases, dict(enumerate(names)))
    wrong = []
    for i, n in enumerate(names):
        _, _, code, fragment = F.CORPUS[n]
        model = F.defect(*F.apply(lay.raw, cases[i][1]))
        rc, msg = hook[i]
        print(f"{base:6s} {n:24s} want {code} '{fragment}': model {model}, program {codes[i]} '{said[str(i)]}', hook {rc} '{msg}'")
        if model != (code, fragment) or codes[i] != code or fragment not in said[str(i)].split(" ", 1)[1] or rc != -code or fragment not in msg:
            wrong.append(n)
    assert not wrong, wrong


# ---- 3. the sweep -----------------------------------------------------------------------------------------------------------
def test_single_field_sweep_agrees_with_the_model(lib, exes, bases, tmp_path):
    """Every 32- and 64-bit field of the header and of every buffer, op and seg record of the fp16 64x64 file, set to 0, 1, v + 1,
    2 v, 2^31 - 1, 2^32 - 1 (and 2^64 - 1024): the program accepts exactly what the model accepts and refuses with the model's
    code; every field a rule mentions is refused at least once; the hook agrees on every accepted case and 1 in 16 of the others.
    (A case that unlinks a block from its fusion group breaks no rule: the hook's group count is not compared.)"""
    t0 = time.time()
    lay = F.Layout(bases["fp16"])
    sw = F.sweep(lay)
    cases = [(i, [edit]) for i, (_, edit) in enumerate(sw)]
    model = [F.defect_edited(lay, [edit]) for _, edit in sw]
    t_model = time.time() - t0
    codes, _ = _program(exes, tmp_path, lay.raw, cases)
    t_program = time.time() - t0 - t_model
    differ = [(sw[i], model[i], codes[i]) for i in range(len(sw)) if (model[i][0] if model[i] else F.OK) != codes[i]]
    assert not differ, differ[:20]
    refused, total = {}, {}
    for (label, _), m in zip(sw, model):
        total[label] = total.get(label, 0) + 1
        refused[label] = refused.get(label, 0) + (m is not None)
    for label in sorted(total):
        print(f"{label:28s} {refused[label]:5d} of {total[label]:5d} refused")
    assert {lb for lb in total if lb not in F.UNRULED and not refused[lb]} == set()       # not vacuous: every ruled field is refused somewhere
    assert {lb for lb in F.UNRULED if refused[lb]} == set()                                  # and no rule hides in a field called free
    rejected = [i for i in range(len(sw)) if model[i] is not None]
    to_hook = [i for i in range(len(sw)) if model[i] is None] + rejected[::16]
    hook = _hook_child(tmp_path, lay.raw, [cases[i] for i in sorted(to_hook)], {i: sw[i] for i in to_hook})
    wrong = [(sw[i], model[i], hook[i]) for i in to_hook if (hook[i][0] >= 0) != (model[i] is None)]
    t_all = time.time() - t0
    print(f"sweep: {len(sw)} cases, {len(rejected)} refused; hook on {len(to_hook)}; model {t_model:.1f} s, program pair {t_program:.1f} s, "
          f"hook child {t_all - t_model - t_program:.1f} s")
    assert not wrong, wrong[:20]
    assert len(sw) > 8000       # on the order of 10^4 single-field cases
