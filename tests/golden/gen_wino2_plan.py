"""Writes tests/golden/wino2_plan.json.gz: what the library answers to the host queries of the 2-D Winograd convolution over the grid of
tests/test_conv_dispatch.py (wino2_plan_table; no GPU needed).  The committed fixture was written by this script against the
libm3d.so of commit 42e02ca, the last one with the A/B-only kernel families and the one-row stem kernel:

    M3D_LIB_PATH=<that build>/libm3d.so python tests/golden/gen_wino2_plan.py --with-one-row-stem-pack

--with-one-row-stem-pack: the library's stem buffer still begins with the one-row kernel's pack (13 row pairs x 6 xi x 64 lanes floats
per 32-channel block); its share is subtracted, so the fixture holds the bytes of the rows pack alone.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_conv_dispatch as T  # noqa: E402

ONE_ROW_PACK_BYTES = 13 * 6 * 64 * 4      # per 32-channel block


def main():
    from m3d import _lib
    L = _lib.lib()
    stem = None
    if "--with-one-row-stem-pack" in sys.argv[1:]:
        def stem(cout):
            return L.m3d_conv3d_stem_wino_packed_weight_bytes(cout) - (cout + 31) // 32 * ONE_ROW_PACK_BYTES
    table = T.wino2_plan_table(L, stem)
    with open(T.PLAN_FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(json.dumps(table, sort_keys=True, separators=(",", ":")).encode())
    print("%s: %d plan rows from %s" % (T.PLAN_FIXTURE, len(table["plans"]), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
