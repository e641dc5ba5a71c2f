"""The lists pred_eval collects per scored pose, under names.

`ScoreLists` is one family of per-pose values for one pose set: {key: lists[cls][iter]} for a fixed key tuple, the layout
lib.dataset.evaluation.PoseEvaluator reads (all_poses_est[cls][iter], errors[key][cls][iter]).  `PairLists` is the same idea for
values kept once per pair, {key: list}.  Both grow by `append` and join another rank's by `extend`, list by list, so a merge over
ranks is `extend` in rank order under every name.  No torch here: the objects travel between ranks by pickle.
"""
from __future__ import print_function, division


class ScoreLists(object):
    def __init__(self, keys, n_cls, n_iter):
        self.keys, self.n_cls, self.n_iter = tuple(keys), int(n_cls), int(n_iter)
        self.lists = {k: [[[] for _ in range(self.n_iter)] for _ in range(self.n_cls)] for k in self.keys}

    def __getitem__(self, key):
        return self.lists[key]

    def append(self, cls, it, values):
        """one pose of class `cls` at iteration `it`: values, one per key"""
        assert len(values) == len(self.keys), (self.keys, len(values))
        for k, v in zip(self.keys, values):
            self.lists[k][cls][it].append(v)

    def extend(self, other):
        assert (other.keys, other.n_cls, other.n_iter) == (self.keys, self.n_cls, self.n_iter), "extend: two different families"
        for k in self.keys:
            for c in range(self.n_cls):
                for it in range(self.n_iter):
                    self.lists[k][c][it].extend(other.lists[k][c][it])


class PairLists(object):
    def __init__(self, keys):
        self.keys = tuple(keys)
        self.lists = {k: [] for k in self.keys}

    def __getitem__(self, key):
        return self.lists[key]

    def append(self, values):
        """one pair: values, one per key"""
        assert len(values) == len(self.keys), (self.keys, len(values))
        for k, v in zip(self.keys, values):
            self.lists[k].append(v)

    def extend(self, other):
        assert other.keys == self.keys, "extend: two different families"
        for k in self.keys:
            self.lists[k].extend(other.lists[k])
