"""Training minibatches from a dataset that stays on the device (csrc/train_sample.hip; DESIGN, "Training samples").

Reference: lib/roi_data/minibatch.py and lib/utils/blob.py:97-202 (prep_im_for_blob, crop_data_3d), the annotation readers of
lib/datasets/soma_dataset.py:197-289 and lib/datasets/nuclei_dataset.py:214-315, and MinibatchSampler of lib/roi_data/loader.py without
aspect grouping.  The reference reads, normalises, searches and crops every sample on the host in every step and ships the fp32 tile;
here the raw uint16 volumes and their boxes are uploaded once, the statistics are computed once per volume, and a step's tiles and
ground-truth boxes are produced by two launches.  The readers and the epoch order are host logic and need no GPU."""
import os

import numpy as np
import torch

from . import ops

__all__ = ["SampleCfg", "Annotations", "read_soma_annotations", "read_nuclei_annotations", "epoch_order", "TrainSet", "Batch"]

_M64 = (1 << 64) - 1
_ORDER_BASE = 1 << 40                 # the keys of an epoch's order: indices far from those of the per-image draws


class SampleCfg:
    """The keys the input path reads; defaults = the nuclei YAML merged over lib/core/config.py."""

    def __init__(self, **kw):
        self.PP_METHOD = "norm1"                            # config.py:31
        self.NEED_CROP = False                              # TRAIN.NEED_CROP
        self.IN_SIZE = (64, 256, 256)                       # TRAIN.IN_SIZE (slices, height, width)
        self.IM_SIZE = (64, 256, 256)                       # TRAIN.IM_SIZE
        self.RADIUS_EXP_RATIO = 0.3                         # TRAIN.RADIUS_EXP_RATIO
        self.IMS_PER_BATCH = 2                              # TRAIN.IMS_PER_BATCH (config.py:56)
        unknown = sorted(set(kw) - set(self.__dict__))
        if unknown:
            raise TypeError("SampleCfg: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(sorted(self.__dict__))))
        self.__dict__.update(kw)
        self.IN_SIZE = tuple(int(v) for v in self.IN_SIZE)
        self.IM_SIZE = tuple(int(v) for v in self.IM_SIZE)
        if self.PP_METHOD != "norm1":
            raise ValueError("SampleCfg: PP_METHOD %r is not built (norm1 only)" % (self.PP_METHOD,))

    @staticmethod
    def nuclei(**kw):
        return SampleCfg(**kw)

    @staticmethod
    def soma(**kw):
        d = dict(NEED_CROP=True, IM_SIZE=(128, 256, 256), RADIUS_EXP_RATIO=0.2)
        d.update(kw)
        return SampleCfg(**d)


class Annotations:
    """One image's ground truth: boxes fp32 [K,6] (x1,y1,z1,x2,y2,z2), classes int32 [K], crowd bool [K], volumes fp32 [K] and, for
    soma, segms fp32 [K,4] (x, y, z, radius)."""

    def __init__(self, boxes, classes, crowd, volumes, segms=None):
        self.boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        self.classes = np.asarray(classes, np.int32).reshape(-1)
        self.crowd = np.asarray(crowd, bool).reshape(-1)
        self.volumes = np.asarray(volumes, np.float32).reshape(-1)
        self.segms = segms

    def __iter__(self):             # boxes, classes, crowd, segms / volumes
        return iter((self.boxes, self.classes, self.crowd, self.segms if self.segms is not None else self.volumes))


def _clean(objs, im_size, segms):
    """_add_gt_annotations: corners from (x1,y1,z1,w,h,s), clipped to the image; an object without volume or without extent goes"""
    S, H, W = im_size
    boxes, crowd, volumes, segs = [], [], [], []
    for bbox, volume, iscrowd, seg in objs:
        lo = [float(v) for v in bbox[:3]]
        hi = [l + max(0.0, e - 1.0) for l, e in zip(lo, bbox[3:])]
        lim = (W - 1.0, H - 1.0, S - 1.0)
        lo = [min(m, max(0.0, v)) for v, m in zip(lo, lim)]
        hi = [min(m, max(0.0, v)) for v, m in zip(hi, lim)]
        if volume > 0 and all(h > l for l, h in zip(lo, hi)):
            boxes.append(lo + hi)
            crowd.append(bool(iscrowd))
            volumes.append(volume)
            segs.append(seg)
    return Annotations(np.array(boxes, np.float32).reshape(-1, 6), np.ones(len(boxes), np.int32), crowd, volumes,
                       np.array(segs, np.float32).reshape(-1, 4) if segms else None)


def _lines(txt):
    if isinstance(txt, (list, tuple)):
        return list(txt)
    with open(txt, "r") as f:
        return f.readlines()


def read_soma_annotations(txt, cfg):
    """soma_dataset.py:197-289.  txt: the path of an annotation file, or its lines; after a header line, `x y z radius` per soma.  The
    centre is clamped into IM_SIZE, the box is the sphere's with its diameter expanded by RADIUS_EXP_RATIO, clamped and truncated."""
    S, H, W = cfg.IM_SIZE
    objs = []
    for a in _lines(txt)[1:]:
        p = a.rstrip().split(" ")
        c = [min(W - 1, int(p[0])), min(H - 1, int(p[1])), min(S - 1, int(p[2]))]
        r = int(p[3])
        half = r * 2 * (1.0 + cfg.RADIUS_EXP_RATIO) / 2.0
        lo = [int(max(v - half, 0.0)) for v in c]
        ext = [int(min(v + half, m - 1)) - l + 1 for v, m, l in zip(c, (W, H, S), lo)]
        objs.append((lo + ext, 4.0 / 3.0 * 3.14159 * r ** 3, 0, c + [r]))
    return _clean(objs, cfg.IM_SIZE, True)


def read_nuclei_annotations(bbox_txt, mask, cfg):
    """nuclei_dataset.py:214-252 and its _add_gt_annotations.  bbox_txt: path or lines; after a header, `id x y z w h s marker` per
    nucleus.  mask: the label volume [S,H,W].  A nucleus's volume is the count of its marker inside its box.  A box that touches the x or
    y border with an extent below 25 there is a crowd (don't-care) region - unless it is the file's last line and no line before it was
    kept as a nucleus."""
    S, H, W = cfg.IM_SIZE
    mask = np.asarray(mask)
    ann = _lines(bbox_txt)[1:]
    objs, valid = [], False
    for a in ann:
        p = a.rstrip().split(" ")
        x1, y1, z1 = min(W - 1, int(float(p[1]))), min(H - 1, int(float(p[2]))), min(S - 1, int(float(p[3])))
        w, h, s, marker = int(float(p[4])), int(float(p[5])), int(float(p[6])), int(p[7])
        volume = int(np.count_nonzero(mask[z1:z1 + s, y1:y1 + h, x1:x1 + w] == marker))
        at_border = ((x1 == 0 or x1 + w - 1 >= W) and w < 25) or ((y1 == 0 or y1 + h - 1 >= H) and h < 25)
        crowd = at_border and (valid or a != ann[-1])
        if not crowd:
            valid = True
        objs.append(([x1, y1, z1, w, h, s], volume, crowd, None))
    return _clean(objs, cfg.IM_SIZE, False)


def _mix(z):
    z = (z * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_order(n, seed, epoch):
    """The order of one epoch: a permutation of range(n) that is a pure function of (seed, epoch) - MinibatchSampler with
    ASPECT_GROUPING: False draws numpy.random.permutation here.  Indices in ascending (key, index), key = the sampling contract's
    key(stream(seed), 2^40 + epoch n + i)."""
    st = _mix(int(seed) & _M64)
    keys = [_mix((st + _ORDER_BASE + epoch * n + i) & _M64) >> 32 for i in range(n)]
    return sorted(range(n), key=lambda i: (keys[i], i))


def _shift_spots(segms, keep, origin, cfg):
    """blob.py:153-161: the centres of the kept spheres move by the crop origin (x, y, z) and are clipped to [0, IN_SIZE - 1], in fp32;
    the radius stays.  Without a crop (NEED_CROP False) crop_data_3d never runs and the spheres pass through."""
    if segms is None:
        return None
    sp = np.array(segms[keep], np.float32).reshape(-1, 4)
    if cfg.NEED_CROP:
        S, H, W = cfg.IN_SIZE
        for a, top in enumerate((W - 1, H - 1, S - 1)):
            sp[:, a] -= np.float32(origin[a])
            np.clip(sp[:, a], 0, top, out=sp[:, a])
    return sp


class Batch:
    """One minibatch.  Device tensors: data fp32 [B,1,s,h,w]; boxes fp32 [B,max_boxes,6] (kept boxes first, in order, then zeros); keep
    int32 [B,max_boxes] (source index of every kept box, then -1); info int32 [B,8] = ox, oy, oz, kept, status, candidates, 0, 0; score
    fp64 [B].  `indices` are the images' dataset indices.  The per-image lists wait for the one host read (info and keep, copied to a
    pinned buffer behind an event when the batch was made); nothing else does."""

    def __init__(self, dataset, indices, data, boxes, keep, info, score, host, event):
        self.indices, self.data, self.boxes, self.keep, self.info, self.score = list(indices), data, boxes, keep, info, score
        self._set, self._host, self._event, self._lists = dataset, host, event, None

    def _read(self):
        if self._lists is None:
            self._event.synchronize()
            B = len(self.indices)
            h = self._host.numpy()
            info, keep = h[:B * 8].reshape(B, 8), h[B * 8:].reshape(B, -1)
            boxes, classes, crowd, spots = [], [], [], []
            for b, i in enumerate(self.indices):
                n = int(info[b, 3])
                k = keep[b, :n]
                boxes.append(self.boxes[b, :n])
                classes.append(self._set.classes[i][k])
                crowd.append(self._set.crowd[i][k])
                spots.append(_shift_spots(self._set.segms[i], k, info[b, :3], self._set.cfg))
            self._lists = (boxes, classes, crowd, info.copy(), spots)
        return self._lists

    @property
    def gt_boxes(self):
        """per image the kept boxes, CUDA fp32 [K_b,6]: what box_head_targets takes"""
        return self._read()[0]

    @property
    def gt_classes(self):
        return self._read()[1]

    @property
    def gt_crowd(self):
        return self._read()[2]

    @property
    def gt_spots(self):
        """per image the spheres (x, y, z, r) of the kept boxes in tile coordinates, host fp32 [K_b,4] (None for a dataset without
        segms): what mask_targets takes with anno_type 'spot'.  Waits for the same host read as gt_boxes."""
        return self._read()[4]

    @property
    def host_info(self):
        return self._read()[3]

    def rpn_boxes(self, b):
        """(gt, dc) of image b as add_rpn_blobs splits them (rpn.py:66-73): the boxes of a class that are no crowd, and the crowd boxes"""
        boxes, classes, crowd = self._read()[:3]
        gt_i, dc_i = np.flatnonzero((classes[b] > 0) & ~crowd[b]), np.flatnonzero(crowd[b])
        if len(dc_i) == 0 and len(gt_i) == len(classes[b]):
            return boxes[b], boxes[b][:0]
        dev = boxes[b].device
        return boxes[b][ops.upload(gt_i, dev)], boxes[b][ops.upload(dc_i, dev)]


class TrainSet:
    """The training images of a dataset, resident on the device.

    volumes: per image a uint16 (or float32) array [D,H,W]; annotations: per image an Annotations (or boxes, classes, crowd); cfg:
    SampleCfg.  Volumes and boxes are uploaded once and each volume's norm1 statistics are computed once; classes, crowd flags and the
    search bounds stay on the host."""

    def __init__(self, volumes, annotations, cfg, device="cuda"):
        if len(volumes) != len(annotations) or not len(volumes):
            raise ops.M3DError("TrainSet: one annotation per volume, and at least one volume")
        self.cfg, self.device = cfg, torch.device(device)
        self.volumes, self.stats, self.boxes, self.classes, self.crowd, self.start_max, self.segms = [], [], [], [], [], [], []
        s, h, w = cfg.IN_SIZE
        for vol, ann in zip(volumes, annotations):
            boxes, classes, crowd = list(ann)[:3]
            boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
            if not len(boxes):
                raise ops.M3DError("TrainSet: an image without boxes (the reference fails on np.min of nothing)")
            if torch.is_tensor(vol):
                v = vol.to(self.device).contiguous()
            else:
                vol = np.ascontiguousarray(vol)
                if vol.dtype not in (np.uint16, np.float32):
                    raise TypeError("TrainSet: volumes are uint16 or float32")
                v = torch.from_numpy(vol).to(self.device)
            D, H, W = (int(x) for x in v.shape)
            self.volumes.append(v)
            self.stats.append(ops.norm1_stats(v))
            self.boxes.append(torch.from_numpy(boxes).to(self.device))
            self.classes.append(np.asarray(classes, np.int32).reshape(-1))
            self.crowd.append(np.asarray(crowd, bool).reshape(-1))
            sg = getattr(ann, "segms", None)
            self.segms.append(None if sg is None else np.ascontiguousarray(sg, np.float32).reshape(-1, 4))
            lo = np.floor(boxes[:, :3].min(axis=0))
            self.start_max.append(tuple(int(min(lo[a], d - n)) for a, d, n in ((0, W, w), (1, H, h), (2, D, s))))   # blob.py:106-114
        self.max_boxes = max(int(b.shape[0]) for b in self.boxes)

    def __len__(self):
        return len(self.volumes)

    @classmethod
    def from_dir(cls, root, dataset, split="train", cfg=None, device="cuda"):
        """The reference's layout under `root` (the directory that holds the split lists and the image directory, DATASETS[..][IM_DIR]
        minus its last component): `{split}.txt` with one name per line, and
          soma:   image/{name}/{name}.tif, annotation {name}.txt                       (soma_dataset.py:167-199)
          nuclei: image/{name}.tif, annotation bbox/{name}.txt and mask/{name}.tif     (nuclei_dataset.py:176-217)
        root: that directory, or (root, image_dir, annotation_dir) where the two are laid out elsewhere."""
        from .io import read_tiff_stack
        if dataset not in ("soma", "nuclei"):
            raise ValueError("TrainSet.from_dir: dataset is 'soma' or 'nuclei'")
        if cfg is None:
            cfg = SampleCfg.soma() if dataset == "soma" else SampleCfg.nuclei()
        if isinstance(root, (tuple, list)):
            root, im_dir, ann_dir = root
        else:
            im_dir, ann_dir = os.path.join(root, "image"), os.path.join(root, "annotation")
        with open(os.path.join(root, split + ".txt"), "r") as f:
            names = [t.rstrip() for t in f.readlines()]
        vols, anns = [], []
        for n in names:
            if dataset == "soma":
                vols.append(read_tiff_stack(os.path.join(im_dir, n, n + ".tif")))
                anns.append(read_soma_annotations(os.path.join(ann_dir, n + ".txt"), cfg))
            else:
                vols.append(read_tiff_stack(os.path.join(im_dir, n + ".tif")))
                anns.append(read_nuclei_annotations(os.path.join(ann_dir, "bbox", n + ".txt"),
                                                    read_tiff_stack(os.path.join(ann_dir, "mask", n + ".tif")), cfg))
        return cls(vols, anns, cfg, device=device)

    def sample(self, indices, seed, fixed_origin=None):
        """The minibatch of the images `indices` on the current stream.  seed: one 64-bit seed per image, or one base seed (image b then
        draws with seed + b).  A pure function of the dataset, the indices and the seeds, bit-identical run to run."""
        idx = [int(i) for i in indices]
        seeds = [int(v) for v in seed] if np.ndim(seed) else [int(seed) + b for b in range(len(idx))]
        B, M = len(idx), self.max_boxes
        meta = torch.empty((B * (8 + M),), dtype=torch.int32, device=self.device)
        data, boxes, keep, info, score = ops.train_sample(
            [(self.volumes[i], self.stats[i], self.boxes[i], self.start_max[i]) for i in idx], self.cfg.IN_SIZE, self.cfg.NEED_CROP, seeds, M,
            fixed_origin=fixed_origin, meta=meta)
        host = torch.empty((B * (8 + M),), dtype=torch.int32, pin_memory=True)
        host.copy_(meta, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return Batch(self, idx, data, boxes, keep, info, score, host, event)

    def batch_plan(self, steps, seed):
        """(indices, seeds) of `steps` minibatches: the whole batches of every epoch's order (BatchSampler with drop_last, as
        tools/train_net_step.py builds it) and, for step t and image b, the seed `seed + 1 + t IMS_PER_BATCH + b`."""
        n, B = len(self), int(self.cfg.IMS_PER_BATCH)
        if n < B:
            raise ops.M3DError("TrainSet: %d images make no minibatch of %d" % (n, B))
        plan, epoch = [], 0
        while len(plan) < steps:
            order = epoch_order(n, seed, epoch)
            for j in range(n // B):
                if len(plan) < steps:
                    t = len(plan)
                    plan.append((order[j * B:(j + 1) * B], [int(seed) + 1 + t * B + b for b in range(B)]))
            epoch += 1
        return plan

    def batches(self, steps, seed, prefetch=1):
        """Yields `steps` minibatches in the reference's order.  prefetch=1 prepares batch t + 1 on a side stream while batch t is
        consumed, so its host read is long done when its lists are asked for; prefetch=0 makes each batch on the current stream when it
        is asked for.  The batches are the same either way."""
        plan = self.batch_plan(steps, seed)
        if not prefetch:
            for idx, seeds in plan:
                yield self.sample(idx, seeds)
            return
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))   # the uploads and statistics of the constructor

        def make(t):
            with torch.cuda.stream(side):
                return self.sample(*plan[t])
        nxt = make(0) if plan else None
        for t in range(len(plan)):
            cur = nxt
            main = torch.cuda.current_stream(self.device)
            main.wait_event(cur._event)                         # the consumer's stream sees the finished tiles
            for x in (cur.data, cur.boxes, cur.keep, cur.score):
                x.record_stream(main)                           # allocated on the side stream, used on this one
            nxt = make(t + 1) if t + 1 < len(plan) else None
            yield cur
