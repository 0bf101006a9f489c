"""CPU: the deferred partial rounds of the Poseidon2 permutation (csrc/poseidon2.hpp, p2_internal_rounds_deferred -- what the bulk
hashing kernels run between the two external round groups) against the round-wise permutation, word for word, on the host.
tests/poseidon2_deferred_cpp.cpp holds the states: all zero, all p-1, one lane p-1 for each lane, alternating 0 / p-1, the values
1, (p-1)/2, (p+1)/2, 2^27 and 2^31 mod p in every lane and alone, and 10 000 seeded random states.  The same program runs once more
as a stand-alone binary under the address and undefined-behaviour sanitizers (the 64-bit accumulators must not overflow a signed
type anywhere, the table must not be read past its end)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "poseidon2_deferred_cpp.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-DZK_NO_HOST_AVX512", "-I", os.path.join(ROOT, "zkvm-prover_amd", "csrc")]
N_STATES = 16 + 2 + 2 + 5 * 33 + 7 + 10000


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++"] + extra + FLAGS + [SRC, "-o", exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_deferred_rounds_equal_the_roundwise_permutation(tmp_path_factory):
    out = _run(_build(tmp_path_factory, "p2d", ["-O2"]))
    assert out == ["ok", str(N_STATES)]


def test_deferred_rounds_under_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "p2d_san", ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
    out = _run(exe)
    assert out == ["ok", str(N_STATES)]
