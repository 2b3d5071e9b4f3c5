"""Child process of tests/test_engine_file_cpu.py: walks a list of damaged engine files through unina_debug_fusable_groups --
the host side of unina_load_engine, which touches no device -- and prints a line per case, so that a crash of the loader names
its case instead of taking pytest down.
  python engine_file_child.py CASES WORK
CASES: engine_file_cases.pack_cases (the base file and, per case, its edits); WORK: a scratch path. The base is written to
WORK once; each case patches its bytes in place, runs the hook, and puts the base's bytes back.
stdout: "BEGIN id" before each call, "END id rc message" after it (rc: the hook's return, -code or the group count)."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_cases(payload):
    assert payload[:8] == b"UNEVAL01"
    (base_len,) = struct.unpack_from("<Q", payload, 8)
    base = payload[16:16 + base_len]
    at = 16 + base_len
    (n,) = struct.unpack_from("<Q", payload, at)
    at += 8
    cases = []
    for _ in range(n):
        cid, n_edits = struct.unpack_from("<II", payload, at)
        at += 8
        edits = [struct.unpack_from("<QIQ", payload, at + 20 * j) for j in range(n_edits)]
        at += 20 * n_edits
        cases.append((cid, edits))
    assert at == len(payload)
    return base, cases


def walk(lib, payload, work, out=sys.stdout):
    base, cases = read_cases(payload)
    with open(work, "wb") as f:
        f.write(base)
    for cid, edits in cases:
        print(f"BEGIN {cid}", file=out, flush=True)
        length = len(base)
        with open(work, "r+b") as f:
            for off, width, value in edits:
                if width == 0:
                    length = value
                else:
                    f.seek(off)
                    f.write(value.to_bytes(8, "little")[:width])
            f.truncate(length)
        rc = lib.unina_debug_fusable_groups(work.encode())
        msg = lib.unina_last_error(None).decode(errors="replace") if rc < 0 else ""
        print(f"END {cid} {rc} {msg}", file=out, flush=True)
        with open(work, "r+b") as f:       # the base again
            if length < len(base):
                f.seek(length)
                f.write(base[length:])
            for off, width, _ in edits:
                if width and off < length:
                    f.seek(off)
                    f.write(base[off:off + width])


if __name__ == "__main__":
    from unina_yolo_dla_amd import engine
    with open(sys.argv[1], "rb") as f:
        walk(engine.load_library(), f.read(), sys.argv[2])
