"""GPU: the DEVICE forms of every primitive of csrc/babybear.hpp and csrc/poseidon2.hpp -- red_2p, msub and canon_signed are inline
assembly there, different text from the host forms -- at boundary operands and at the stated precondition limits, against the
Python-integer reference of field_probe_ref.py, and exhaustively (stride 1: all 2^32 words for red_2p, every d in (-p, p) for canon_signed,
every x in [0, p) for center_signed, mhalve, mdouble, mdiv_pow2<2|3|4|8|27>, sbox7 and the to_monty/from_monty round trip) against the
plain `%` forms beside them.  tests/field_probe.hip is built here with hipcc for gfx950 and run once, as a child process under a time
limit."""
import subprocess
import time

import pytest

import field_probe_ref as ref

pytestmark = pytest.mark.gpu


def test_device_forms_at_boundary_operands_and_exhaustively(tmp_path):
    exe = tmp_path / "field_probe_gpu"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "-I", ref.CSRC, ref.SRC, "-o", str(exe)])
    t0 = time.time()
    seen = ref.run_probe(exe, tmp_path, 1, timeout=180)
    print("device probe: %.1f s, %d jobs" % (time.time() - t0, len(seen)))
    for name in ref.OPS:
        assert any(k == name or k.startswith(name + "[") for k in seen), name
    assert seen["exhaustive red_2p"] == 1 << 32 and seen["exhaustive canon_signed"] == 2 * ref.P - 1 and seen["exhaustive sbox7"] == ref.P
    assert sum(1 for k in seen if k.startswith("exhaustive")) == 12
