"""Writes tests/golden/product_bits.npz: what every form of the monolithic product gives, on an MI355X, for the seeded inputs of
tests/test_gpu_product_bits.py (which holds the cases, the forms and the recording itself: ``record``).  The committed file was
recorded with the last commit before the product's kernels were built from shared pieces ("Krylov iteration: skip zero dv
values, the empty column, the second q"; its hash is in the file as ``commit``), through that commit's shim.  Running this again
records whatever the library of the checkout gives: do that only to pin a deliberate change of the product's arithmetic.

    python tests/golden/make_product_bits.py [commit hash to store]
"""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import conftest  # noqa: E402
import test_gpu_product_bits as pb  # noqa: E402


def main():
    if len(sys.argv) > 1:
        commit = sys.argv[1]
    else:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    case = conftest.prepare_case("cylinder", conftest.GOLDEN / "cylinder" / "cylinder.h5", tempfile.mkdtemp(prefix="product_bits_"))
    out = pb.record(case)
    np.savez_compressed(pb.GOLDEN, commit=np.array(commit), **out)
    print(pb.GOLDEN, pb.GOLDEN.stat().st_size, "bytes,", len(out), "arrays, commit", commit)


if __name__ == "__main__":
    main()
