"""``python -m classpose_amd.entrypoints.train_head``: fine-tune the 1x1 semantic class head of a checkpoint on the device with
everything else frozen -- the reference's ``--freeze backbone segmentation_head neck`` training mode
(paper_experiments/run_training.py:92-98,354-358) reduced to arrays of fixed-size crops.

    python -m classpose_amd.entrypoints.train_head --images X.npy --labels Y.npy --pretrained_model CKPT \\
        --n_epochs 100 --batch_size 8 --save_path DIR --model_name NAME --device cuda:0 [--augment hed_only --scale_range 0.5]

Images are ``(N, 256, 256, 3)`` uint8 (normalised per crop like inference does) or ``(N, 3, 256, 256)`` float32 (already
normalised); labels ``(N, 256, 256)`` integer class maps with -100 where nothing is annotated.  The result is an ordinary
checkpoint in the reference's key layout: ``predict_wsi`` and ``ClassposeModel`` load it unchanged.
"""
from __future__ import annotations

import argparse

import numpy as np

from ..log import get_logger

logger = get_logger(__name__)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train the 1x1 semantic class head on the device with the backbone frozen")
    p.add_argument("--images", required=True, help=".npy, (N,256,256,3) uint8 or (N,3,256,256) float32")
    p.add_argument("--labels", required=True, help=".npy, (N,256,256) integer class maps, -100 = not annotated")
    p.add_argument("--test_images", default=None)
    p.add_argument("--test_labels", default=None)
    p.add_argument("--pretrained_model", required=True, help="checkpoint (state dict) to adapt")
    p.add_argument("--nclasses", type=int, default=None, help="class count of a NEW head when the checkpoint has none")
    p.add_argument("--n_epochs", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--learning_rate", type=float, default=5e-5)
    p.add_argument("--weight_decay", type=float, default=0.1)
    p.add_argument("--class_weights", type=float, nargs="+", default=None)
    p.add_argument("--nimg_per_epoch", type=int, default=None)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--cache_features", action=argparse.BooleanOptionalAction, default=True,
                   help="run the frozen backbone once per crop and train from the cached neck features")
    p.add_argument("--augment", default=None, choices=["hed_only", "geometry", "enhanced"],
                   help="augment every training batch on the device: hed_only = stain jitter + flip / rotation / scale / crop, "
                        "geometry = the latter alone (enhanced is not built)")
    p.add_argument("--scale_range", type=float, default=0.5, help="random scale in [1 - r/2, 1 + r/2] (with --augment)")
    p.add_argument("--augment_label_fill", type=int, default=0,
                   help="class of pixels the warp takes from outside the crop: 0 = background as in the reference, -100 = not annotated")
    p.add_argument("--save_only_trainable_params", action="store_true")
    p.add_argument("--random_seed", type=int, default=42)
    p.add_argument("--save_path", required=True)
    p.add_argument("--model_name", required=True)
    p.add_argument("--device", default="cuda:0")
    return p


def main(args) -> None:
    from ..train import HeadTrainer, train_class_head
    if (args.test_images is None) != (args.test_labels is None):
        raise SystemExit("--test_images and --test_labels go together")
    images, labels = np.load(args.images), np.load(args.labels)
    test_images = np.load(args.test_images) if args.test_images else None
    test_labels = np.load(args.test_labels) if args.test_labels else None
    trainer = HeadTrainer(args.pretrained_model, nclasses=args.nclasses, device=args.device, precision=args.precision,
                          class_weights=args.class_weights, weight_decay=args.weight_decay)
    path, train_losses, test_losses = train_class_head(
        trainer, images, labels, test_images, test_labels, batch_size=args.batch_size, n_epochs=args.n_epochs,
        learning_rate=args.learning_rate, nimg_per_epoch=args.nimg_per_epoch, cache_features=args.cache_features,
        save_path=args.save_path, model_name=args.model_name, random_seed=args.random_seed,
        augment=args.augment, scale_range=args.scale_range, label_fill=args.augment_label_fill)
    if args.save_only_trainable_params:
        trainer.save(path, save_only_trainable_params=True)
    logger.info(f"final train loss {train_losses[-1]:.4f}" + (f", test loss {test_losses[-1]:.4f}" if test_images is not None else ""))
    print(path)


if __name__ == "__main__":
    main(build_parser().parse_args())
