"""Box-and-mask validation metrics with the reference's names (utils/segment/metrics.py): host numpy, once per validation run, on top of
`metrics.ap_per_class` -- the statistics themselves come from the device (segment_val.SegValStats).

    fitness(x)                                   0.1 mAP@0.5 + 0.9 mAP@0.5:0.95 of the box AND of the mask columns of an (N, 8+) array
    ap_per_class_box_and_mask(tp_m, tp_b, ...)   {'boxes': {p, r, ap, f1, ap_class}, 'masks': {...}}
    Metric / Metrics                             per-class results and their means, Metrics = (box Metric, mask Metric)
"""
from __future__ import annotations

import numpy as np

from .metrics import ap_per_class

_FITNESS_W = np.array([0.0, 0.0, 0.1, 0.9, 0.0, 0.0, 0.1, 0.9])


def fitness(x):
    """x (N, 8+): [P, R, mAP@0.5, mAP@0.5:0.95] of the boxes then of the masks -> (N,) weighted sum."""
    return (np.asarray(x)[:, :8] * _FITNESS_W).sum(1)


def ap_per_class_box_and_mask(tp_m, tp_b, conf, pred_cls, target_cls, plot=False, save_dir=".", names=()):
    """ap_per_class over the mask and the box true positives of the same predictions."""
    out = {}
    for key, tp in (("boxes", tp_b), ("masks", tp_m)):
        p, r, f1, ap, ap_class = ap_per_class(tp, conf, pred_cls, target_cls, plot=plot, save_dir=save_dir, names=names)[2:]
        out[key] = {"p": p, "r": r, "ap": ap, "f1": f1, "ap_class": ap_class}
    return out


class Metric:
    """Per-class precision, recall, F1 and AP (nc, niou) of one kind (boxes or masks)."""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = [], [], [], [], []

    @property
    def ap50(self):
        return self.all_ap[:, 0] if len(self.all_ap) else []

    @property
    def ap(self):
        return self.all_ap.mean(1) if len(self.all_ap) else []

    @property
    def mp(self):
        return self.p.mean() if len(self.p) else 0.0

    @property
    def mr(self):
        return self.r.mean() if len(self.r) else 0.0

    @property
    def map50(self):
        return self.all_ap[:, 0].mean() if len(self.all_ap) else 0.0

    @property
    def map(self):
        return self.all_ap.mean() if len(self.all_ap) else 0.0

    def mean_results(self):
        return self.mp, self.mr, self.map50, self.map

    def class_result(self, i):
        return self.p[i], self.r[i], self.ap50[i], self.ap[i]

    def get_maps(self, nc):
        """(nc,) AP@0.5:0.95 per class; classes without data get the mean."""
        maps = np.zeros(nc) + self.map
        for i, c in enumerate(self.ap_class_index):
            maps[c] = self.ap[i]
        return maps

    def update(self, results):
        """results: (p, r, ap, f1, ap_class) -- the order of ap_per_class_box_and_mask's dict values."""
        self.p, self.r, self.all_ap, self.f1, self.ap_class_index = results


class Metrics:
    """The box and the mask Metric of one validation run."""

    def __init__(self):
        self.metric_box = Metric()
        self.metric_mask = Metric()

    def update(self, results):
        self.metric_box.update(list(results["boxes"].values()))
        self.metric_mask.update(list(results["masks"].values()))

    def mean_results(self):
        return self.metric_box.mean_results() + self.metric_mask.mean_results()

    def class_result(self, i):
        return self.metric_box.class_result(i) + self.metric_mask.class_result(i)

    def get_maps(self, nc):
        """Per-class box mAP plus mask mAP, elementwise -- what the reference returns (utils/segment/metrics.py)."""
        return self.metric_box.get_maps(nc) + self.metric_mask.get_maps(nc)

    @property
    def ap_class_index(self):
        return self.metric_box.ap_class_index
