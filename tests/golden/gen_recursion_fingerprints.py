"""Writes tests/golden/recursion_fingerprints.json: the circuits and witnesses that tests/test_recursion_fingerprint_cpu.py pins.
Run on a commit whose circuits are the ones to keep (python tests/golden/gen_recursion_fingerprints.py); a change of
zkvm-prover_amd/csrc/recursion.hip that is meant to leave the circuits alone must NOT need this file written again."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib  # noqa: E402
import test_recursion_fingerprint_cpu as t  # noqa: E402

if __name__ == "__main__":
    oracle_lib.lib()
    forms = t.build_forms(oracle_lib)
    out = {}
    for name in t.FORMS:
        out[name], serial = t.fingerprint(forms[name])
        assert serial == out[name]["witness"]["full"], name
    with open(t.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", t.GOLDEN)
