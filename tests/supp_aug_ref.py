"""Shared by tests/golden/make_golden_supp_aug.py (fixture writer) and the query augmentation tests (fixture readers): the inputs of
the `suppaug` cases, the merge step in torch (generalized_rcnn.py:280-288: two lines) and numpy closed forms of the merge kernels."""
import numpy as np

AUG = 2            # NUM_SUPP_AUG + 1 of every fixture: the support and its horizontal flip, the dataset's supp_aug=True rows

# (method, case of golden_utils.CASES, shared backbone) of the forward fixtures case_suppaug_<method>_<case>.npz /
# case_suppaug_shared_<method>_<case>.npz
FORWARD_CASES = [("avg", "small", False), ("max", "small", False), ("avg", "nonsquare", False), ("max", "nonsquare", False),
                 ("avg", "shots5", False), ("max", "shots5", False), ("max", "small", True)]
# (method, case, supp_roialign) of the training fixtures train_suppaug_<method>_<case>.npz.  supp_roialign False: the reference's query
# pooling has a CPU backward there, so the fixture also holds the reference's OWN gradients of both backbones (`refgrad.*`), through
# torch's max backward; True: the reference's gradients with the pooled vector detached (`refgrad_detached.*`).  Every fixture holds
# the oracle's full gradients (`fullgrad_oracle.*`), which were held against the reference's before anything was written.
TRAIN_CASES = [("avg", "small", True), ("max", "small", True), ("max", "nonsquare", False)]
BOX_CASE = ("max", "small")       # box_suppaug_max_small.npz: the reference's full eval forward, roi_heads included


def forward_name(method, case, shared):
    return "case_suppaug_%s%s_%s.npz" % ("shared_" if shared else "", method, case)


def train_name(method, case):
    return "train_suppaug_%s_%s.npz" % (method, case)


def aug_queries(q):
    """[N,3,h,w] -> [N*2,3,h,w]: every query followed by its horizontal flip (coco.py:343-349), numpy or torch"""
    if isinstance(q, np.ndarray):
        return np.ascontiguousarray(np.stack([q, q[..., ::-1]], axis=1).reshape((-1,) + q.shape[1:]))
    import torch
    return torch.stack([q, q.flip(-1)], dim=1).reshape((-1,) + tuple(q.shape[1:])).contiguous()


def case_inputs(case):
    """(images [B,3,H,W], queries [B*S*AUG,3,h,w]) float32 numpy: the case's inputs with every query made a group"""
    import golden_utils as gu
    img, q = gu.case_inputs(case)
    return img, aug_queries(q)


def merge(feat, aug, method, group_dim=0):
    """generalized_rcnn.py:281,285-288 on one level: [G*aug, ...] -> [G, ...] (torch)"""
    grouped = feat.reshape((feat.shape[0] // aug, aug) + tuple(feat.shape[1:]))
    return grouped.mean(dim=1) if method == "avg" else grouped.max(dim=1)[0]


def avg_closed_form(x, aug):
    """x numpy fp32 [G*aug, ...] -> the members added in member order in fp32, then ONE true division by np.float32(aug)"""
    g = x.reshape((x.shape[0] // aug, aug) + x.shape[1:])
    s = g[:, 0].copy()
    for a in range(1, aug):
        s = s + g[:, a]
    return (s / np.float32(aug)).astype(np.float32)


def within_one_ulp(got, ref):
    """numpy fp32 arrays: |got - ref| <= the spacing of fp32 at |ref|"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ulp = np.nextafter(np.abs(ref), np.float32(np.inf)) - np.abs(ref)
    return bool((np.abs(got - ref) <= ulp).all())
