#!/usr/bin/env python3
"""Train TinyYolo on Prophesee recordings: ``PropheseeFeed`` -> ``TinyYolo`` -> ``FlatTrainer``, one loss per step.

    python tools/train_on_recordings.py --data-dir ./data --dataset gen1 --steps 100 --batch-size 4 --num-steps 42

expects ``<data-dir>/<dataset>/train/*_bbox.npy`` with their ``*_td.dat``.  ``--augment`` switches the event augmentation
on (flip, zoom with shift, random drop); ``--label-steps K`` trains on every labelled timestep (multi-target samples and
``SODa(label_steps=K)``).  The feed of step n+1 is queued while step n runs.  No checkpoint logic beyond FlatTrainer's.
``--ema-decay D`` keeps a weight average inside the optimiser step (``--ema-warmup``: its ramp), ``--warmup-steps W`` warms
the learning rate up over W steps and lets it fall along a cosine over the rest, and ``--val-batches N`` ends the run with
``validation_step`` over N batches of ``<data-dir>/<dataset>/val``: once on the live weights and, with an average, once
under ``averaged_weights()`` - both sets of mAP keys are printed.
``--chained`` (with ``--label-steps K``) trains on CONSECUTIVE windows with the neuron state carried from step to step:
``PropheseeFeed(chained=True)`` binds every batch slot to one recording, ``SODa(carry_state=True)`` keeps the detached
state and resets the slots that open a new recording; no random prefix is cut (``time_window=0``).
``--representation {binary,count,time,voxel}`` (with ``--rep-clip N``, ``--rep-scale S``) chooses what a cell of the event
frames holds (``EventRepresentation``), for the training and the validation feed alike."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import snn_for_object_detection_amd as S  # noqa: E402
from snn_for_object_detection_amd.trainer import FlatTrainer, warmup_cosine  # noqa: E402

MAP_KEYS = ("map", "map_50", "mar_1", "mar_10", "mar_100")


def validate(model, batches):
    """``validation_step`` over ``batches`` in eval mode -> mean loss and the mAP keys (the caller restores train mode)."""
    model.eval()
    losses = []
    with torch.no_grad():
        for batch in batches:
            losses.append(model.validation_step(batch).detach())
    model.on_validation_epoch_end()
    out = {"val_loss": float(torch.stack(losses).mean())}
    out.update({k: float(model.logged[k]) for k in MAP_KEYS})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--dataset", default="gen1", choices=("gen1", "1mpx"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--num-steps", type=int, default=42)
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--label-steps", type=int, default=None, metavar="K")
    ap.add_argument("--cls-loss", default="ce", choices=("ce", "focal"))
    ap.add_argument("--focal-gamma", type=float, default=2.0)
    ap.add_argument("--box-loss", default="l1", choices=("l1", "giou", "diou", "ciou"))
    ap.add_argument("--box-loss-weight", type=float, default=1.0)
    ap.add_argument("--assigner", default="iou", choices=("iou", "tal"),
                    help="which anchors are positives: the static IoU rule or the task-aligned assigner")
    ap.add_argument("--chained", action="store_true",
                    help="consecutive windows per batch slot, neuron state carried across steps (needs --label-steps)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D", help="weight average with this decay (off)")
    ap.add_argument("--ema-warmup", type=int, default=2000, help="time constant, in updates, of the decay ramp")
    ap.add_argument("--warmup-steps", type=int, default=0, metavar="W",
                    help="learning rate: linear warmup over W steps, then a cosine down to 1 %% at --steps (constant)")
    ap.add_argument("--val-batches", type=int, default=0, metavar="N", help="validate on N batches of the val split at the end")
    ap.add_argument("--representation", default="binary", choices=S.EventRepresentation.KINDS,
                    help="what a cell of the event frames holds: a flag, an event count, a time surface, a voxel grid")
    ap.add_argument("--rep-clip", type=int, default=None, metavar="N", help="clip of count / voxel cells (none)")
    ap.add_argument("--rep-scale", type=float, default=1.0, metavar="S", help="factor on the cell values")
    args = ap.parse_args()
    representation = S.EventRepresentation(args.representation, clip=args.rep_clip, scale=args.rep_scale)
    if args.chained and args.label_steps is None:
        ap.error("--chained needs --label-steps K (chained windows carry six-column labels)")
    carried = dict(carry_state=True, time_window=0) if args.chained else {}

    augment = S.EventAugment(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1), seed=args.seed) if args.augment else None
    feed = S.PropheseeFeed(args.data_dir, dataset=args.dataset, split="train", batch_size=args.batch_size,
                           num_steps=args.num_steps, one_label=args.label_steps is None, seed=args.seed, augment=augment,
                           chained=args.chained, representation=representation)
    torch.manual_seed(args.seed)
    model = S.TinyYolo(num_classes=len(feed.get_labels()), label_steps=args.label_steps, cls_loss=args.cls_loss,
                       focal_gamma=args.focal_gamma, box_loss=args.box_loss,
                       box_loss_weight=args.box_loss_weight, assigner=args.assigner, **carried).cuda().train()
    lr = warmup_cosine(args.lr, args.warmup_steps, args.steps) if args.warmup_steps > 0 else args.lr
    trainer = FlatTrainer(model, lr=lr, ema_decay=args.ema_decay, ema_warmup=args.ema_warmup)
    batch = next(feed)
    for step in range(args.steps):
        trainer.zero_grad()
        loss = model.training_step(batch)
        loss.backward()
        trainer.step()
        batch = next(feed)          # queued behind the step that is still running
        print(f"step {step:5d}  loss {float(loss.detach()):.6f}", flush=True)
    if args.val_batches > 0:
        val = S.PropheseeFeed(args.data_dir, dataset=args.dataset, split="val", batch_size=args.batch_size,
                              num_steps=args.num_steps, one_label=args.label_steps is None, seed=args.seed,
                              chained=args.chained, representation=representation)
        batches = [next(val) for _ in range(args.val_batches)]
        trainer.synchronize()
        print("val live    ", validate(model, batches), flush=True)
        if args.ema_decay is not None:
            with trainer.averaged_weights():
                print("val averaged", validate(model, batches), flush=True)
        model.train()


if __name__ == "__main__":
    main()
