"""CPU: the HOST forms of every primitive of csrc/babybear.hpp and csrc/poseidon2.hpp at boundary operands and at the stated
precondition limits, against the Python-integer reference of field_probe_ref.py (exact value or congruence, and the promised range of
the raw word).  tests/field_probe.hip is built with plain g++; the device forms (inline assembly) are test_gpu_field_probe.py's.

The exhaustive unary passes (fast form against a plain `%` form, which is itself checked against Python on the sampled operands) run on
every HOST_STRIDE-th operand here: a sample of about 35 million operands per pass (61 is odd, so the walk is not locked to one class of the
low bits), twelve passes; the device test walks every operand."""
import os
import subprocess
import time

import pytest

import field_probe_ref as ref

HOST_STRIDE = 61


@pytest.fixture(scope="module")
def probe_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("field_probe") / "field_probe_cpu"
    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", ref.CSRC, ref.SRC, "-o", str(exe)])
    return exe


def test_reference_permutation_matches_pymodel():
    ref.cross_check_permutation_with_pymodel()


def test_boundary_set_holds_what_the_kernels_never_see():
    b, p = set(ref.B), ref.P
    assert {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, ref.MONTY_ONE, p - ref.MONTY_ONE, ref.MONTY_R2, 1 << 27, 15 << 27, 1 << 30,
            0x2AAAAAAA, 0x55555555 % p, 0x77FFFFFF, 0x78000000} <= b
    assert ref.MONTY_ONE == 0x0FFFFFFE and ref.MONTY_R2 == 1172168163


def test_host_forms_at_boundary_operands(probe_exe, tmp_path):
    exe = probe_exe
    t0 = time.time()
    seen = ref.run_probe(exe, tmp_path, HOST_STRIDE, timeout=600)
    print("host probe: %.1f s, %d jobs, %d sampled operands" % (time.time() - t0, len(seen), sum(v for k, v in seen.items() if not k.startswith("exhaustive"))))
    for name in ref.OPS:
        assert any(k == name or k.startswith(name + "[") for k in seen), name   # no primitive dropped from the job list
    assert sum(1 for k in seen if k.startswith("exhaustive")) == 12


def test_probe_refuses_files_it_cannot_bound(probe_exe, tmp_path):
    """Sizes are checked before anything runs: a job that claims more operands than the file holds is refused, not read past its end."""
    import struct

    exe = probe_exe
    big = [ref.MAGIC, 1, 1, ref.OP["red_2p"], ref.OP["plain_red_2p"], 0, 0, 0, 2, 0xFFFFFFFF, 0]   # 2^33 operands at stride 2^32 - 1
    for words in (big, [ref.MAGIC, 1, 0, ref.OP["mmul"], 5, 1, 2], [ref.MAGIC, 1, 0, 9999, 1, 1], [ref.MAGIC, 1, 0, ref.OP["lazyacc"], 1, 0, 0, 0, 0, 1 << 30],
                  [ref.MAGIC, 1, 1, ref.OP["mmul"], ref.OP["plain_identity"], 0, 0, 4, 0, 1, 0], [ref.MAGIC, 2, 0, ref.OP["mneg"], 1, 3]):
        src = tmp_path / "bad.bin"
        src.write_bytes(struct.pack("<%dI" % len(words), *words))
        r = subprocess.run([str(exe), str(src), str(tmp_path / "bad.out")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "field_probe:" in r.stderr, (words, r.returncode, r.stderr)
        assert not os.path.exists(tmp_path / "bad.out")
