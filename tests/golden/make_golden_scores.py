#!/usr/bin/env python3
"""Golden fixture of the regression score table (Utils.py:118-175 calc_metrics) by IMPORTING THE REAL REFERENCE (dev container only).
Uses the stubs of make_golden.py and writes one new file:

    python tests/golden/make_golden_scores.py      # scores_ref.npz

For the two input pairs of tests.scores_ref (random: labels on the MOSI grid, predictions = labels + noise; crafted: the half-to-even
cases, the clips and beyond, labels and predictions at 0.0 and -0.0) it stores the fp32 inputs and the eight outputs of the reference's
calc_metrics(y_true, y_pred), the call of Solver.get_score_from_result (Solver.py:385-386), evaluated on the float64 copies of those
values.  Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as MG  # noqa: E402,F401  (puts the reference, with its stubs, in front of sys.path)
from tests import scores_ref as SR  # noqa: E402
from mimrl_amd.Utils import REGRESSION_SCORE_KEYS  # noqa: E402

import Utils as RU  # noqa: E402  (reference)


if __name__ == "__main__":
    out = {}
    for tag, (p, y) in (("random", SR.random_pair()), ("crafted", SR.crafted_pair())):
        # float64 copies of the committed fp32 values: the table as a function of the values, free of the fp32 rounding of np.mean / np.corrcoef
        s = RU.calc_metrics(y.astype(np.float64).reshape(-1, 1), p.astype(np.float64).reshape(-1, 1), to_print=False)
        assert tuple(s) == REGRESSION_SCORE_KEYS, list(s)
        out[f"{tag}_pred"], out[f"{tag}_y"] = p, y
        out[f"{tag}_scores"] = np.array([s[k] for k in REGRESSION_SCORE_KEYS], np.float64)
        print(tag, " ".join(f"{k}={float(s[k]):.6f}" for k in s))
    path = os.path.join(HERE, "scores_ref.npz")
    np.savez_compressed(path, **out)
    print(f"scores_ref: wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
