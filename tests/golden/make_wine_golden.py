"""Generates tests/golden/wine_seed_0.npz: the six arrays of upstream's datasets/wine/wine_seed_0.npz exactly as stored
(features f32, labels int32), so that the tests need no dataset directory.  Data only.  Run:
    python tests/golden/make_wine_golden.py DATASET_DIR
with DATASET_DIR laid out like upstream's datasets/ folder, i.e. holding wine/wine_seed_0.npz (default:
$GMMVI_DATASET_DIR).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = ("features_train", "labels_train", "features_test", "labels_test", "features_vali", "labels_vali")


def main(dataset_dir):
    with np.load(os.path.join(dataset_dir, "wine", "wine_seed_0.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in ARRAYS}
    out = os.path.join(HERE, "wine_seed_0.npz")
    np.savez_compressed(out, **arrays)
    for key, a in arrays.items():
        print(f"{key}: {a.shape} {a.dtype}")
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    d = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GMMVI_DATASET_DIR")
    if not d:
        sys.exit("usage: make_wine_golden.py DATASET_DIR (or set GMMVI_DATASET_DIR)")
    main(d)
