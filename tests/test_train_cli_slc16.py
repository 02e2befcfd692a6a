"""tools/train.py --rna_slc 16 is an argparse error without --resident (the host-weight engine's weight gradient takes Z <= 4), and the
message says so; nothing is imported that needs a GPU before the arguments are checked."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rna_slc_16_needs_resident():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--rna_slc", "16", "--data", "d", "--out", "o"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--resident" in r.stderr and "Z <= 4" in r.stderr, (r.returncode, r.stderr)
