"""tests/golden/make_ref_calls.py -- writes tests/golden/ref_calls_<i>.npz: runs tests/test_oracle_vs_reference.py against the reference's own kernels
compiled for the CPU (oracle/_ref: oracle.build_ref() where the reference sources are present) with every call recorded (tests/_ref_replay.py).
Run it again after a change to the inputs of those tests."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pytest  # noqa: E402

import oracle  # noqa: E402
from _ref_replay import GOLDEN, Recorder  # noqa: E402


def main():
    live = oracle.ref_ops("fma")
    if live is None:
        sys.exit("oracle/_ref is not built (oracle.build_ref() needs the reference sources)")
    rec = Recorder(live, oracle.ops())
    oracle.ref_ops = lambda tag="fma": rec if tag == "fma" else None
    rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_reference.py")])
    if rc != 0:
        sys.exit(f"the tests failed against the live reference (pytest exit {rc}): nothing written")
    rec.save(GOLDEN)
    for f in sorted(os.listdir(GOLDEN)):
        if f.startswith("ref_calls_"):
            print(f"{f}: {os.path.getsize(os.path.join(GOLDEN, f))} bytes")


if __name__ == "__main__":
    main()
