"""One-shot detection end to end on an MI355X with this build, the way a user of RyanXLi/OneshotDet would call it:

    python examples/detect.py [--checkpoint model_0040000.pth | --c2 R-50.pkl] [--dtype bf16|f32] [--second-stage]
                              [--shared-backbone] [--no-supp-roialign] [--box-cls-loss ce_loss|focal_loss|mse_loss|l1_loss|cxe_loss]
                              [--soft-labeling]       # the model was trained with FEW_SHOT.SOFT_LABELING (needed for l1_loss / cxe_loss)
                              [--classes K]           # the class sweep: K categories per image in one pass, one merged BoxList per image
                              [--gallery G]           # the query gallery: enroll G supports once, then detect image batches against the bank
    python examples/detect.py --checkpoint model_0930.pth --shared-backbone --no-supp-roialign      # the 0930 model

  * weights: a reference `.pth` (utils/checkpoint.py format), a Detectron ResNet `.pkl` for the backbones, or — there is no
    network here — the deterministic synthetic weights the tests use;
  * model: a checkpoint is run as the model that wrote it (shared backbone when it holds no `supp_backbone.*`);
    --shared-backbone (FEW_SHOT.SIAMESE_BACKBONE False) for the other sources.  --no-supp-roialign (FEW_SHOT.SUPP_ROIALIGN False)
    pools the query pyramid by global average: the reference's default config and configs/fcos/0930fixed_thres.yaml need it
    with --shared-backbone, and nothing in a weights file says so (a training checkpoint of this build records it);
  * inputs: lists of CHW BGR-minus-mean images of different sizes for targets and queries; `to_image_list` pads them to
    a common /32 size and keeps the true sizes (data/collate_batch.py + structures/image_list.py of the reference);
  * output: one BoxList per target image (boxes, scores, labels = the query's class id), like `GeneralizedRCNN.forward`;
  * --classes K: every image is asked about K categories at once (K supports per image, `target_ids` = K ids per image): the target
    backbone runs once per image, and the BoxList of an image holds the detections of all K categories in descending score order;
  * --gallery G: the deployment form of the sweep.  `det.enroll(supports, labels)` runs the query branch ONCE for G categories and
    returns a QueryBank; every later `det(images, bank, target_ids=...)` runs no query backbone at all.  target_ids names, per image,
    the labels to look for (None: all G).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import checkpoint, layers, modules, spec, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--c2", default="")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--first-stage-only", action="store_true")
    ap.add_argument("--shared-backbone", action="store_true", help="one backbone for target and query (SIAMESE_BACKBONE False)")
    ap.add_argument("--no-supp-roialign", action="store_true", help="pool the query pyramid by global average (SUPP_ROIALIGN False)")
    ap.add_argument("--soft-labeling", action="store_true",
                    help="the model was trained with IoU soft labels (FEW_SHOT.SOFT_LABELING): admits l1_loss (scored like mse_loss) "
                         "and cxe_loss (scored like ce_loss)")
    ap.add_argument("--box-cls-loss", default=spec.BOX_CLS_LOSS, choices=list(spec.BOX_CLS_LOSSES + spec.BOX_CLS_LOSSES_SOFT),
                    help="second-stage classification loss the model was trained with (FEW_SHOT.SECOND_STAGE_CLS_LOSS): "
                         "the sigmoid losses have one class logit and a sigmoid score")
    ap.add_argument("--linear-fusion", action="store_true",
                    help="the model was trained with FEW_SHOT.LINEAR_FUSION: no compress_dim_conv, a 512-channel feature_aggreg.0")
    ap.add_argument("--neg-support", action="store_true",
                    help="the model was trained with a negative support (FEW_SHOT.NEG_SUPPORT; 'ce_loss', no --linear-fusion): "
                         "validated, detection itself does not change")
    ap.add_argument("--classes", type=int, default=1,
                    help="K: ask every image about K categories in one pass (the class sweep, detect(..., classes=K)); the supports "
                         "are synthetic here")
    ap.add_argument("--gallery", type=int, default=0,
                    help="G: enroll G synthetic supports once (OneShotDetector.enroll) and detect three batches of images against the "
                         "bank, each asking for its own labels")
    ap.add_argument("--supp-aug", type=int, default=1, metavar="N",
                    help="the model was trained with query augmentation groups (FEW_SHOT.SUPP_AUG, NUM_SUPP_AUG = N - 1): every support "
                         "is passed as N consecutive rows, here the support and its horizontal flip in turn")
    ap.add_argument("--supp-aug-method", default="avg", choices=list(spec.SUPP_AUG_METHODS), help="FEW_SHOT.SUPP_AUG_METHOD")
    args = ap.parse_args()
    supp_aug, supp_aug_method = spec.supp_aug_mode(args.supp_aug, args.supp_aug_method, args.neg_support and not args.first_stage_only)

    def groups(supports):
        """every support -> its group of supp_aug consecutive rows: the support, its horizontal flip, the support, ..."""
        return [s if a % 2 == 0 else s.flip(-1) for s in supports for a in range(supp_aug)]
    siamese = not args.shared_backbone
    roialign = not args.no_supp_roialign
    if args.checkpoint:
        siamese = checkpoint.has_query_backbone(args.checkpoint)       # the file's own mode
    # the model's options (spec.MODEL_OPTIONS), once: the detector's, and those among them that decide the state_dict's shapes
    options = dict(siamese_backbone=siamese, supp_roialign=roialign, box_cls_loss=args.box_cls_loss, soft_labeling=args.soft_labeling,
                   linear_fusion=args.linear_fusion, neg_support=args.neg_support)
    shape_options = {name: options[name] for name in spec.SHAPE_OPTIONS}
    shapes = spec.hot_path_shapes(siamese) if args.first_stage_only else spec.full_model_shapes(**shape_options)
    defaults = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes).items()}
    if args.checkpoint:
        sd, extras = checkpoint.load_checkpoint(args.checkpoint, defaults=defaults, **shape_options)
        print("loaded", args.checkpoint, "(%s backbone)" % ("siamese" if siamese else "shared"),
              {k: v for k, v in extras.items() if not isinstance(v, dict)})
        if "box_cls_loss" in extras and str(extras["box_cls_loss"]) != args.box_cls_loss and not args.first_stage_only:
            raise SystemExit("%s was trained with box_cls_loss=%r: pass --box-cls-loss %s" % (
                args.checkpoint, extras["box_cls_loss"], extras["box_cls_loss"]))
        if "supp_roialign" in extras and bool(extras["supp_roialign"]) != roialign:
            raise SystemExit("%s was trained with supp_roialign=%r: %s --no-supp-roialign" % (
                args.checkpoint, bool(extras["supp_roialign"]), "drop" if roialign is False else "add"))
    elif args.c2:
        sd = checkpoint.load_c2_resnet(args.c2, defaults, **shape_options)
        print("backbones initialised from", args.c2)
    else:
        sd = defaults
        print("synthetic weights (no checkpoint given)")
    if args.first_stage_only:
        options.update(linear_fusion=False, neg_support=False)
    det = modules.OneShotDetector(sd, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32,
                                 supp_aug=supp_aug, supp_aug_method=supp_aug_method, **options)
    # two targets and two queries of different sizes
    targets = [torch.from_numpy(synth.make_images("ex.t%d" % i, 1, h, w)[0]) for i, (h, w) in enumerate([(480, 640), (512, 384)])]
    queries = [torch.from_numpy(synth.make_images("ex.q%d" % i, 1, h, w)[0]) for i, (h, w) in enumerate([(127, 127), (96, 160)])]
    images = layers.to_image_list(targets, size_divisible=spec.SIZE_DIVISIBILITY)
    images_supp = layers.to_image_list(groups(queries), size_divisible=spec.SIZE_DIVISIBILITY)
    print("padded batch", tuple(images.tensors.shape), "true sizes", images.image_sizes)
    if args.gallery > 0:
        G = args.gallery
        sizes = [(127, 127), (96, 160)]
        supports = [torch.from_numpy(synth.make_images("ex.g%d" % g, 1, *sizes[g % 2])[0]) for g in range(G)]
        labels = [1 + (7 * g) % 80 for g in range(G)]
        bank = det.enroll(layers.to_image_list(groups(supports), size_divisible=spec.SIZE_DIVISIBILITY), labels)       # the query branch, once
        print("enrolled %d gallery slots, labels %s" % (bank.slots, labels))
        K = min(3, G)
        for step in range(3):                                    # a stream of image batches against the same bank
            batch = [torch.from_numpy(synth.make_images("ex.t%d.%d" % (step, i), 1, h, w)[0]) for i, (h, w) in enumerate([(480, 640), (512, 384)])]
            # step 0 asks for every label; later steps for K labels per image of their own
            ids = None if step == 0 else [[labels[(step + b + k) % G] for k in range(K)] for b in range(2)]
            results = det(layers.to_image_list(batch, size_divisible=spec.SIZE_DIVISIBILITY), bank, target_ids=ids)
            torch.cuda.synchronize()
            for i, bl in enumerate(results):
                got = bl.get_field("labels").cpu().tolist()
                print("batch %d image %d: %s for labels %s, top score %.3f (label %s)" % (
                    step, i, bl, "all" if ids is None else ids[i], float(bl.get_field("scores")[0]) if len(bl) else float("nan"),
                    got[0] if got else "-"))
        return
    if args.classes > 1:
        # K supports per image, row b*K + k = category slot k of image b (synthetic: no two alike), and K class ids per image
        K = args.classes
        sizes = [(127, 127), (96, 160)]
        supports = [torch.from_numpy(synth.make_images("ex.q%d.%d" % (b, k), 1, *sizes[(b + k) % 2])[0]) for b in range(2) for k in range(K)]
        images_supp = layers.to_image_list(groups(supports), size_divisible=spec.SIZE_DIVISIBILITY)
        ids = [[1 + (17 * b + k) % 80 for k in range(K)] for b in range(2)]
        results = det(images, images_supp, target_ids=ids)
        torch.cuda.synchronize()
        for i, bl in enumerate(results):
            labels = bl.get_field("labels").cpu().tolist()
            per_class = {c: labels.count(c) for c in ids[i]}
            print("image %d: %s merged from %d categories, per category %s, top score %.3f (label %s)" % (
                i, bl, K, per_class, float(bl.get_field("scores")[0]) if len(bl) else float("nan"), labels[0] if labels else "-"))
        return
    results = det(images, images_supp, target_ids=[17, 3])
    torch.cuda.synchronize()
    for i, bl in enumerate(results):
        s = bl.get_field("scores")
        print("image %d: %s, top score %.3f, label %s" % (i, bl, float(s[0]) if len(bl) else float("nan"),
                                                          int(bl.get_field("labels")[0]) if bl.has_field("labels") and len(bl) else "-"))


if __name__ == "__main__":
    main()
