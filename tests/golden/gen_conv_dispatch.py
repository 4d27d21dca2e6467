"""Writes tests/golden/conv_dispatch.json.gz: what the conv dispatch of THIS checkout asks of the library over the grid of
tests/test_conv_dispatch.py (no GPU needed).  The committed fixture was written by this script on the commit before
m3d/conv_plan.py existed:

    python tests/golden/gen_conv_dispatch.py
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

import test_conv_dispatch as T  # noqa: E402


def main():
    with pytest.MonkeyPatch.context() as mp:
        rec = T.record_all(mp)
    with open(T.FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode())       # (400 KB of JSON; `zcat | python -m json.tool` reads it)
    print("%s: %d cases, %d units rows" % (T.FIXTURE, len(rec["cases"]), len(rec["zw_units"])))


if __name__ == "__main__":
    main()
