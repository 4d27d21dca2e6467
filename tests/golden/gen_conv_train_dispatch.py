"""Writes tests/golden/conv_train_dispatch.json.gz: what m3d.compat.conv3d and its backward of THIS checkout ask of the library over
the grid of tests/test_conv_train_dispatch.py (no GPU needed).  The committed fixture was written by this script on the commit before
conv_plan.plan_train_conv existed; on a later commit it must write the same bytes:

    python tests/golden/gen_conv_train_dispatch.py
"""
import gzip
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_conv_train_dispatch as T  # noqa: E402


def main():
    with pytest.MonkeyPatch.context() as mp:
        rec = T.record_all(mp)
    with open(T.FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode())
    print("%s: %d records, %d through torch" % (T.FIXTURE, len(rec), sum(r["forward"] == "torch" for r in rec.values())))


if __name__ == "__main__":
    main()
