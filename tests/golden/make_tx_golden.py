"""Records tests/golden/tx/*.npz: the seeded inputs of tests/tx_cases.py and
what the reference's own modOneSymbol / modRefSymbol make of them (compiled
from the reference tree by tx_cases.build_ref_harness; needs that tree).
tests/test_tx_ref_cpu.py asserts that the committed files equal a fresh run.

    python tests/golden/make_tx_golden.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tx_cases  # noqa: E402


def main():
    if not tx_cases.reference_present():
        sys.exit("the reference tree is absent: nothing recorded")
    os.makedirs(tx_cases.GOLDEN_TX, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for rows, C, prefix in tx_cases.REF_SHAPES:
            path = tx_cases.fixture_path(rows, C, prefix)
            np.savez(path, **tx_cases.reference_record(tmp, rows, C, prefix))
            print(f"{path}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
