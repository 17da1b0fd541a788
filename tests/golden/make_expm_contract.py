"""Writes tests/golden/expm_contract.npz: the 50-digit values of the matrix function's contract (tests/expm_cases.py) -- for every
generator its 4 x 4 matrix, its lengths and expm(fl(Q t)) as a double plus a double remainder; for the JC69 closed form its
lengths and (diagonal, remainder, off-diagonal, remainder).  Numbers only.  Prints the NumPy restatement's E_REF0 per generator,
the constants committed in tests/expm_cases.py.

    python tests/golden/make_expm_contract.py            (about ten seconds; needs mpmath)
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import expm_cases as X  # noqa: E402


if __name__ == "__main__":
    data = X.contract()
    for name in X.NAMES:
        e = X.measure_e_ref0(name, data['Q/' + name], data['t/' + name], data['hi/' + name], data['lo/' + name])
        print("E_REF0[%-7s] = %8.3f u   (committed %g)" % (name, e, X.E_REF0[name]))
    print("S_MAX = %d, ||Q t||_1 <= %.6g" % (X.S_MAX, X.NORM_MAX))
    path = os.path.join(X.GOLDEN, "expm_contract.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
