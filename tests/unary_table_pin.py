"""The bits of the unary tables that the GPU tests already make, pinned: tests/golden/unary_table_hashes.json holds the SHA-256 of each table as the
library of the commit named in that file computed it on an MI355X.  The tests that compare a table with the oracle to a tolerance (test_gpu_unary_patches.py:
check, test_gpu_unary.py, test_gpu_dice.py) also call assert_pinned, so that a change which is meant to leave the tables alone -- a kernel moved to another
unit, an argument block reshaped -- shows that it did.  A change that is meant to move bits records the file again and says so."""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unary_table_hashes.json")
_pins = None


def table_hash(U):
    return hashlib.sha256(np.ascontiguousarray(U)).hexdigest()


def key(family, case, kind="univariate", D=1, sim=2, rows=0, sampler="rays", sg_order=None):
    """the parameters of the call that made the table, as one string"""
    k = "%s %s %s D=%d sim=%d rows=%d %s" % (family, case, kind, D, sim, rows, sampler)
    return k if sg_order is None else k + " sg_order=%d" % sg_order


def assert_pinned(U, k):
    global _pins
    if _pins is None:
        with open(PATH) as f:
            _pins = json.load(f)["tables"]
    assert k in _pins, "no pinned hash for the table %r" % k
    assert table_hash(U) == _pins[k], "the bits of the table %r changed" % k
