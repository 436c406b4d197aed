"""Writes tests/golden/chi2inv95_reference.npy: the reference's chi2inv95 table (src/odometry/util.hpp:23, 201 values
"computed in Matlab as chi2inv(0.95, 0:99)") as float64, so that tests/test_oracle_ekf.py checks the generated table
(scripts/gen_chi2_table.py) against it wherever the tests run.  Usage:
    python tests/golden/make_chi2_fixture.py <reference checkout>
"""
import os
import re
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chi2inv95_reference.npy")

text = open(os.path.join(sys.argv[1], "src", "odometry", "util.hpp")).read()
vals = np.array([float(x) for x in re.search(r"chi2inv95 = \{([^}]*)\}", text).group(1).split(",")], np.float64)
assert vals.shape == (201,)
np.save(OUT, vals)
print(OUT, os.path.getsize(OUT), "bytes", vals.shape)
