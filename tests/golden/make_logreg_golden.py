"""Generates tests/golden/logreg_datasets.npz: the two raw tables of the logistic-regression targets exactly as np.loadtxt
reads upstream's files (fp64), so that the tests need no dataset directory.  Data only.  Run:
    python tests/golden/make_logreg_golden.py DATASET_DIR
with DATASET_DIR holding upstream's breast_cancer.data and german.data-numeric (default: $GMMVI_DATASET_DIR).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"breast_cancer": "breast_cancer.data", "german_credit": "german.data-numeric"}


def main(dataset_dir):
    tables = {key: np.loadtxt(os.path.join(dataset_dir, name)).astype(np.float64) for key, name in FILES.items()}
    out = os.path.join(HERE, "logreg_datasets.npz")
    np.savez_compressed(out, **tables)
    for key, t in tables.items():
        print(f"{key}: {t.shape}")
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    d = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GMMVI_DATASET_DIR")
    if not d:
        sys.exit("usage: make_logreg_golden.py DATASET_DIR (or set GMMVI_DATASET_DIR)")
    main(d)
