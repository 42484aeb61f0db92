"""Training end to end on MI355X with this build, the way `tools/train_net.py` + `engine/trainer.py:do_train` of
RyanXLi/OneshotDet drive it (both stages, SGD with the reference's parameter groups, periodic checkpoints, resume):

    python examples/train.py [--iters 20] [--batch 2] [--dtype bf16|f32] [--first-stage-only] [--out /tmp/osd_run]
                             [--shared-backbone]        # one backbone for target and query (SIAMESE_BACKBONE False)
                             [--no-supp-roialign]       # the query pyramid pooled by global average (SUPP_ROIALIGN False)
                             [--no-center-sample]       # positives inside the whole box (FCOS.CENTER_SAMPLE False)
                             [--loc-loss-type giou|iou|linear_iou]      # the regression loss (FCOS.LOC_LOSS_TYPE)
                             [--box-cls-loss ce_loss|focal_loss|mse_loss|l1_loss|cxe_loss]   # the second stage's classification loss
                             [--soft-labeling] [--soft-labeling-func discrete|linear|transLinear|trans4thLinear]   # IoU soft labels
                                                        # (FEW_SHOT.SOFT_LABELING): mse_loss is held against them, l1_loss / cxe_loss need them
                             [--lr-steps 60000,90000,120000] [--lr-gamma 0.1] [--warmup-iters 100] [--warmup-factor 0.3333]
                             [--warmup-method constant|linear]      # the learning-rate schedule (SOLVER.STEPS, GAMMA, WARMUP_*);
                                                        # default: the yaml of record's.  --constant-lr: no schedule, 0.0005 throughout
    python examples/train.py --no-center-sample --loc-loss-type iou ...    # the loss of the reference's defaults (defaults.py:309-311)
    python examples/train.py --shared-backbone --no-supp-roialign ...      # the 0930 model (configs/fcos/0930fixed_thres.yaml)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train.py ...      # one rank per GPU

  * data: `dataset.FewShotCocoDataset` (= the reference's COCODataset: one item per (category, image), seeded epoch order,
    targets of the item's category, support crops of OTHER images' largest objects above the area threshold) over a synthetic
    COCO-format annotation set — there are no datasets here, so the "photos" are random uint8 images of different sizes;
  * input pipeline: `transforms.build_transforms` (Resize / flip / ToTensor / Normalize of the reference, executed by the
    fused device kernels), boxes follow their image; `transforms.collate(..., stem_dtype)` = BatchCollator straight into the
    stem conv's input format;
  * step: `TrainEngine.train_step` = forward + FCOS loss + second-stage loss + backward + (N > 1: bucketed RCCL all-reduce
    behind the backward pass) + SGD + weight repack, at the rate of `solver.LRSchedule` (= WarmupMultiStepLR, tools/train_net.py:80-81)
    for the step's iteration;
  * checkpoints: `checkpoint.save_training_checkpoint` writes the reference's `{"model", "optimizer", "scheduler", "iteration"}`
    format (reference parameter names, momentum included); `--resume` continues from `last_checkpoint`, the schedule at the
    restored iteration.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import checkpoint, dataset, solver, spec, synth, train, transforms as T  # noqa: E402


def synthetic_coco(rng, n_images=24, n_categories=3):
    """A COCO-format annotation set over synthetic uint8 "photos" of different sizes (1 - 3 objects each): what the reference
    reads from instances_*.json, for `dataset.FewShotCocoDataset` = its COCODataset (category catalog, seeded epoch order,
    per-item category, targets, support crops by area threshold)."""
    images, anns, pix = [], [], {}
    for k in range(n_images):
        h, w = int(rng.randint(300, 480)), int(rng.randint(400, 640))
        images.append({"id": k + 1, "file_name": "synthetic_%d" % (k + 1), "height": h, "width": w})
        pix[k + 1] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for _ in range(int(rng.randint(1, 4))):
            x0, y0 = float(rng.uniform(0, w * 0.6)), float(rng.uniform(0, h * 0.6))
            bw, bh = float(rng.uniform(40, w * 0.35)), float(rng.uniform(40, h * 0.35))
            anns.append({"id": len(anns) + 1, "image_id": k + 1, "category_id": int(rng.randint(1, n_categories + 1)),
                         "bbox": [x0, y0, bw, bh], "area": bw * bh, "iscrowd": 0})
    return {"images": images, "annotations": anns, "categories": [{"id": c + 1, "name": "c%d" % c} for c in range(n_categories)]}, pix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2, help="images per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--first-stage-only", action="store_true")
    ap.add_argument("--out", default="/tmp/osd_example_run")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--checkpoint-period", type=int, default=10)
    ap.add_argument("--shared-backbone", action="store_true", help="one backbone for target and query (SIAMESE_BACKBONE False)")
    ap.add_argument("--no-supp-roialign", action="store_true", help="pool the query pyramid by global average (SUPP_ROIALIGN False)")
    ap.add_argument("--no-center-sample", action="store_true", help="positives inside the whole box (FCOS.CENTER_SAMPLE False)")
    ap.add_argument("--loc-loss-type", default=spec.LOC_LOSS_TYPE, choices=list(spec.LOC_LOSS_TYPES),
                    help="regression loss (FCOS.LOC_LOSS_TYPE): 1 - giou, -log(iou) or 1 - iou")
    ap.add_argument("--box-cls-loss", default=spec.BOX_CLS_LOSS, choices=list(spec.BOX_CLS_LOSSES + spec.BOX_CLS_LOSSES_SOFT),
                    help="second-stage classification loss (FEW_SHOT.SECOND_STAGE_CLS_LOSS); the sigmoid losses have one class logit; "
                         "l1_loss / cxe_loss need --soft-labeling")
    ap.add_argument("--soft-labeling", action="store_true", help="IoU soft labels for the second stage (FEW_SHOT.SOFT_LABELING)")
    ap.add_argument("--soft-labeling-func", default=spec.SOFT_LABELING_FUNC, choices=list(spec.SOFT_LABELING_FUNCS),
                    help="soft label as a function of the IoU (FEW_SHOT.SOFT_LABELING_FUNC)")
    ap.add_argument("--linear-fusion", action="store_true",
                    help="box head: one 3x3 conv over cat(x, query) in front of fc6, no compress_dim_conv (FEW_SHOT.LINEAR_FUSION)")
    ap.add_argument("--neg-support", action="store_true",
                    help="second stage: score the sampled ROIs against a support of another category too and add the margin loss "
                         "loss_cls_suppress (FEW_SHOT.NEG_SUPPORT; 'ce_loss', one shot, no --linear-fusion).  The reference ships no "
                         "rule for choosing the negative support (its dataset's negative category is always -1); this example's own "
                         "rule: sample i's negative support is the support crop of sample (i + 1) mod batch")
    ap.add_argument("--supp-aug", type=int, default=1, metavar="N",
                    help="query augmentation groups (FEW_SHOT.SUPP_AUG, NUM_SUPP_AUG = N - 1): every support is N consecutive rows merged "
                         "behind the query backbone.  Here 1 (off), 2 (the crop and its horizontal flip, the dataset's supp_aug=True) or "
                         "4 (NUM_SUPP_AUG 3: crop, flip and the colour-jittered crop and flip, the dataset's num_supp_aug=3)")
    ap.add_argument("--supp-aug-method", default="avg", choices=list(spec.SUPP_AUG_METHODS), help="FEW_SHOT.SUPP_AUG_METHOD")
    rec = solver.LRSchedule.of_record()
    ap.add_argument("--lr-steps", default=",".join(str(m) for m in rec.milestones), help="iterations at which the rate is multiplied by "
                    "--lr-gamma, comma separated (SOLVER.STEPS); '' = none")
    ap.add_argument("--lr-gamma", type=float, default=rec.gamma, help="SOLVER.GAMMA")
    ap.add_argument("--warmup-iters", type=int, default=rec.warmup_iters, help="SOLVER.WARMUP_ITERS")
    ap.add_argument("--warmup-factor", type=float, default=rec.warmup_factor, help="SOLVER.WARMUP_FACTOR")
    ap.add_argument("--warmup-method", default=rec.warmup_method, choices=["constant", "linear"], help="SOLVER.WARMUP_METHOD")
    ap.add_argument("--constant-lr", action="store_true", help="no schedule: the base rate from the first step to the last")
    args = ap.parse_args()
    schedule = None if args.constant_lr else solver.LRSchedule(
        rec.base_lr, tuple(int(m) for m in args.lr_steps.split(",") if m.strip()), args.lr_gamma, args.warmup_factor, args.warmup_iters,
        args.warmup_method)
    # the model's options (spec.MODEL_OPTIONS), once: for the engine and, on --resume, as what the checkpoint is expected to hold
    options = dict(siamese_backbone=not args.shared_backbone, supp_roialign=not args.no_supp_roialign,
                   center_sample=not args.no_center_sample, loc_loss_type=args.loc_loss_type, box_cls_loss=args.box_cls_loss,
                   soft_labeling=args.soft_labeling, soft_labeling_func=args.soft_labeling_func,
                   linear_fusion=args.linear_fusion and not args.first_stage_only, neg_support=args.neg_support)
    # refused here, by name: l1_loss / cxe_loss without --soft-labeling, --neg-support in a combination it does not exist in
    spec.check_options("the example", not args.first_stage_only, **options)
    supp_aug, supp_aug_method = spec.supp_aug_mode(args.supp_aug, args.supp_aug_method, args.neg_support)
    if supp_aug not in (1, 2, 4):
        raise SystemExit("--supp-aug %d: the dataset yields a support crop and its horizontal flip (supp_aug=True), which is --supp-aug 2, "
                         "or both and their colour-jittered versions (num_supp_aug=3), which is --supp-aug 4; the reference has no "
                         "NUM_SUPP_AUG for another group size" % supp_aug)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    shapes = spec.hot_path_shapes(options["siamese_backbone"]) if args.first_stage_only else spec.full_model_shapes(
        **{name: options[name] for name in spec.SHAPE_OPTIONS})

    def make_engine(sd):
        return train.TrainEngine(sd, dtype=dtype, lr=rec.base_lr, second_stage=not args.first_stage_only, lr_schedule=schedule,
                                 supp_aug=supp_aug, supp_aug_method=supp_aug_method, **options)
    start = 0
    last = os.path.join(args.out, "last_checkpoint")
    if args.resume and os.path.exists(last):
        # a first-stage-only run says nothing about the second stage's options: whatever the file holds
        expected = {name: None if args.first_stage_only and spec.MODEL_OPTIONS[name].scope == "second_stage" else value
                    for name, value in options.items()}
        eng, start = checkpoint.resume_training(open(last).read().strip(), make_engine, **expected)
        print("resumed at iteration", start)
    else:
        eng = make_engine(synth.make_state_dict(shapes))      # or checkpoint.load_checkpoint / load_c2_resnet, see detect.py
    eng.defer_join = True
    if world > 1:
        # RCCL AFTER the engine's streams have their hardware queues (profiles/r3_live_exchange.md: the other order cost 14 %
        # of the step), then the bucketed gradient exchange on the engine's update stream
        import torch.distributed as dist
        eng.warm_streams()
        dist.init_process_group("nccl", device_id=torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0"))))
        eng.attach_exchange(dist.group.WORLD)
    tf_img, tf_supp = T.build_transforms(min_size=480, max_size=800, supp_min_size=128, supp_max_size=192, is_train=True)
    coco, pix = synthetic_coco(np.random.RandomState(1234))                # the same annotation set on every rank
    ds = dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], is_train=True, shot=1, supp_area_threshold=40 * 40,
                                    supp_aug=supp_aug == 2, num_supp_aug=3 if supp_aug == 4 else None)
    os.makedirs(args.out, exist_ok=True)
    for it in range(start, args.iters):
        imgs, supps, targets = [], [], []
        for b in range(args.batch):
            item = ds[((it * world + rank) * args.batch + b) % len(ds)]       # DistributedSampler's split: every rank its own items
            dimg, tgt = T.DeviceImage(item["img"]), item["target"]
            # the Compose's Resize and flip steps (Normalize is fused into the collation below)
            for t in tf_img.transforms[:2]:
                dimg, tgt = t(dimg, tgt)
            imgs.append(dimg); targets.append(tgt)
            # the support crop (coco.py:341); with --supp-aug 2 followed by its flip (coco.py:343-349), with --supp-aug 4 also by the
            # colour-jittered crop and flip (coco.py:447-452; DeviceImages already, made by one kernel call): one group of consecutive rows
            for crop in item["img_supp"][:supp_aug]:
                supp = crop if isinstance(crop, T.DeviceImage) else T.DeviceImage(crop)
                for t in tf_supp.transforms[:2]:
                    supp, _ = t(supp, None)
                supps.append(supp)
        images = T.collate(imgs, spec.SIZE_DIVISIBILITY, stem_dtype=dtype)
        queries = T.collate(supps, spec.SIZE_DIVISIBILITY, stem_dtype=dtype)
        # the same crops rotated by one: the same padded shape as `queries`, which the engine requires
        neg_queries = T.collate(supps[1:] + supps[:1], spec.SIZE_DIVISIBILITY, stem_dtype=dtype) if args.neg_support else None
        g = max(len(t) for t in targets)
        gt = torch.zeros(args.batch, g, 4)
        for i, t in enumerate(targets):
            gt[i, :len(t)] = t.bbox
        cnt = torch.tensor([len(t) for t in targets], dtype=torch.int32)
        losses = eng.train_step(images, queries, gt.cuda(), cnt.cuda(), neg_queries=neg_queries)
        if rank == 0 and (it % 5 == 0 or it + 1 == args.iters):
            l = losses.float().cpu()
            extra = "" if eng.box_losses is None else "  loss_classifier %.4f  loss_box_reg %.4f" % tuple(eng.box_losses[:2].float().cpu())
            if eng.box_suppress_loss is not None:
                extra += "  loss_cls_suppress %.4f" % float(eng.box_suppress_loss[0])
            print("iter %4d  lr: %.6f  loss_cls %.4f  loss_reg %.4f  loss_centerness %.4f  (%d positives)%s"      # trainer.py:114,125
                  % (it, eng.lr, l[0], l[1], l[2], int(l[3]), extra))
        if rank == 0 and ((it + 1) % args.checkpoint_period == 0 or it + 1 == args.iters):
            path = os.path.join(args.out, "model_%07d.pth" % (it + 1))
            checkpoint.save_training_checkpoint(path, eng, it + 1)
            print("saved", path)
    eng.join()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
