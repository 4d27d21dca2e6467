#!/usr/bin/env python3
"""Scores label volumes as the reference's tools/evaluation/ scripts do, on the GPU (m3d.evaluate):

  python tools/evaluate.py soma PRED_DIR GT_DIR [--iou-thresh 0.3] [--names a b ...]
        pred/{name}.tif + pred/{name}.npy against gt/{name}/{name}.tif (eval_instance_segmentation_soma.py; names default to the
        entries of GT_DIR, as its __main__ does)
  python tools/evaluate.py nuclei-det RES_DIR SRC_DIR TEST_TXT [--track 02] [--ovthresh 0.4] [--score-thresh 0.4] [--npy]
        evaluation_nuclei_f1score.py: {name}.pkl (or .npy) detections against {SRC_DIR}/{track}_GT/BBOX/bbox_NNN.txt
  python tools/evaluate.py nuclei-seg RES_DIR SRC_DIR TEST_TXT [--track 02] [--ovthresh 0.4] [--pkl]
        evaluation_nuclei_f1score_seg.py: {name}.tif + {name}.npy against {SRC_DIR}/{track}_GT/SEG/man_segNNN.tif
  python tools/evaluate.py soma-dsn PRED_DIR GT_DIR [--iou-thresh 0.3] [--names a b ...]
        eval_instance_segmentation_soma_ngps.py, flag DSN: the connected components of the voxelwise segmentation pred/{name}.tif as
        instances, against gt/{name}/{name}.tif
  python tools/evaluate.py soma-ngps SWC_DIR GT_DIR [--iou-thresh 0.3] [--names a b ...]
        the same script, flag NGPS: the NeuroGPS soma list swc/{name}.swc painted as spheres
Prints the figures the reference scripts print."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("soma", "soma-dsn", "soma-ngps"):
        s = sub.add_parser(name)
        s.add_argument("pred_dir")
        s.add_argument("gt_dir")
        s.add_argument("--iou-thresh", type=float, default=0.3)
        s.add_argument("--names", nargs="*")
    for name in ("nuclei-det", "nuclei-seg"):
        n = sub.add_parser(name)
        n.add_argument("res_dir")
        n.add_argument("src_dir")
        n.add_argument("test_txt")
        n.add_argument("--track", default="02")
        n.add_argument("--ovthresh", type=float, default=0.4)
        if name == "nuclei-det":
            n.add_argument("--score-thresh", type=float, default=0.4)
            n.add_argument("--npy", action="store_true", help="read {name}.npy instead of {name}.pkl")
        else:
            n.add_argument("--pkl", action="store_true", help="read boxes from {name}.pkl instead of {name}.npy")
    a = ap.parse_args(argv)
    from m3d import evaluate as E
    if a.cmd == "soma":
        names = a.names if a.names else sorted(os.listdir(a.gt_dir))
        res = E.eval_instance_segmentation_soma(a.pred_dir, a.gt_dir, names, iou_thresh=a.iou_thresh)
        for name, v in zip(names, res["per_image_ap"]):
            print("img {}: ap {}".format(name, v))
        print("ap: {}".format(res["ap"]))
    elif a.cmd in ("soma-dsn", "soma-ngps"):
        from m3d import evaluate_baselines as EB
        names = a.names if a.names else sorted(os.listdir(a.gt_dir))
        res = EB.eval_instance_segmentation_soma("DSN" if a.cmd == "soma-dsn" else "NGPS", a.pred_dir, a.gt_dir, names,
                                                 iou_thresh=a.iou_thresh)
        for name, v in zip(names, res["per_image_ap"]):
            print("img {}: ap {}".format(name, v))
        print("ap: {}".format(res["ap"]))
    elif a.cmd == "nuclei-det":
        r = E.nuclei_detection_f1(a.res_dir, a.src_dir, a.test_txt, track=a.track, ovthresh=a.ovthresh, score_thresh=a.score_thresh,
                                  save_as_pkl=not a.npy)
        print("done, detection f1 score is {}, precision is {}, recall is {}".format(r["f1"], r["precision"], r["recall"]))
    else:
        r = E.nuclei_segmentation_f1(a.res_dir, a.src_dir, a.test_txt, track=a.track, ovthresh=a.ovthresh, save_as_pkl=a.pkl)
        print("done, instance segmentation f1 score is {:.5f}, precision is {:.5f}, recall is {:.5f}".format(r["f1"], r["precision"],
                                                                                                         r["recall"]))


if __name__ == "__main__":
    main()
