#!/usr/bin/env python3
"""Connected components of a whole TIFF stack as an instance-label stack, on the GPU (m3d.label_components, csrc/label3d.hip):

  python tools/label_volume.py IN.tif OUT.tif [--connectivity 26] [--min-voxels N]

IN.tif: a foreground mask or a semantic segmentation (uint8 / uint16); voxels of equal non-zero value that touch (6, 18 or 26
neighbours) form one instance, as skimage.measure.label does.  --min-voxels drops smaller components and renumbers the rest in the
same order.  OUT.tif is uint16; more than 65 535 components is an error that names the count.  Prints K and the five largest sizes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--connectivity", type=int, default=26, choices=(6, 18, 26))
    ap.add_argument("--min-voxels", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import m3d
    from m3d.io import read_tiff_stack, write_tiff_stack
    labels, K, counts = m3d.label_components(read_tiff_stack(a.input), a.connectivity, return_counts=True)
    if a.min_voxels > 0 and K:
        keep = counts >= a.min_voxels
        keep[0] = False
        new = torch.cumsum(keep.to(torch.int64), 0) * keep                       # old id -> new id (0: dropped), order preserved
        labels = new[labels.long()].to(torch.int32)
        sizes = counts[keep]
        K = int(sizes.numel())
    else:
        sizes = counts[1:]
    if K > 65535:
        raise SystemExit("label_volume: K = %d components do not fit the uint16 output (raise --min-voxels)" % K)
    write_tiff_stack(a.output, labels.cpu().numpy().astype("uint16"))
    top = torch.sort(sizes, descending=True).values[:5].cpu().tolist() if K else []
    print("K: {}".format(K))
    print("largest: {}".format(" ".join(str(int(v)) for v in top)))


if __name__ == "__main__":
    main()
