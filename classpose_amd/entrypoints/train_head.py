"""``python -m classpose_amd.entrypoints.train_head``: fine-tune the 1x1 semantic class head of a checkpoint on the device with
everything else frozen -- the reference's ``--freeze backbone segmentation_head neck`` training mode
(paper_experiments/run_training.py:92-98,354-358) reduced to arrays of fixed-size crops.

    python -m classpose_amd.entrypoints.train_head --images X.npy --labels Y.npy --pretrained_model CKPT \\
        --n_epochs 100 --batch_size 8 --save_path DIR --model_name NAME --device cuda:0 [--augment hed_only --scale_range 0.5] \\
        [--instances I.npy --auto_class_weights --oversampling_method custom --rescale --min_train_masks 1] [--train_neck] [--train_blocks K [--grad_precision bf16 [--attn_grad_precision bf16]] [--train_embed] [--layer_drop 0.4]]
    python -m classpose_amd.entrypoints.train_head --data_path DIR [--test_data_path DIR] [--train_fraction 0.8] \
        [--subsample_fraction F] --pretrained_model CKPT --augment hed_only ... (everything else as above)

A checkpoint whose class head is the reference's UNet (``out_class.encoder_blocks.*`` keys) trains with the same flags
(``classpose_amd.train_unet``); ``--feature_transformation_structure C1 C2 ...`` (at most 4 levels) puts a freshly initialised UNet
head on a checkpoint's backbone instead, with ``--nclasses`` when the checkpoint has no classes.

Images are ``(N, 256, 256, 3)`` uint8 (normalised per crop like inference does) or ``(N, 3, 256, 256)`` float32 (already
normalised); labels ``(N, 256, 256)`` integer class maps with -100 where nothing is annotated.  The result is an ordinary
checkpoint in the reference's key layout: ``predict_wsi`` and ``ClassposeModel`` load it unchanged.

With ``--instances`` (``(N, 256, 256)`` integer instance maps aligned with ``--labels``) one device pass over both maps
(``classpose_amd.dataset_stats``) yields what the reference derives from its datasets: class weights (``--auto_class_weights``),
oversampling probabilities (``--oversampling_method custom``), cell diameters (``--rescale``) and mask counts
(``--min_train_masks``).  The reference's ``run_training.py`` has class weights and ``custom`` oversampling ON by default; here all
four are opt-in, so that a command line without them trains exactly as before.

``--instances_from_labels [--instance_connectivity {4,8}]`` is for semantic-only sets, one class per pixel and no cell ids: the
instance maps are the connected regions of one class, labelled on the device from ``--labels`` (and ``--test_labels``) by
``dataset_stats.instances_from_classes`` -- the reference's recipe for such sets (``ndimage.label`` per class,
paper_experiments/run_cellpose_semantic.py:89-100) -- and then used exactly as if ``--instances`` had been given.  Touching cells
of one class merge into one instance.  ``--split_touching_cells [--split_min_distance D] [--split_min_radius R]`` cuts them apart on
the device (``ops.split_touching``): the peaks of each region's exact squared distance map that lie at least R pixels
(default 2) inside it and that nothing within D pixels (default 5) beats are seeds, and every pixel goes to the nearest seed of its
own region -- straight cuts, no flooding.

``--data_path`` is the reference's data directory instead of the three arrays: ``images.npy`` with ``(H, W, 3)`` images of ANY size
(an object array when they differ) and ``labels.npy`` with ``(H, W, 2)`` maps, channel 0 = instance, channel 1 = class
(``classpose_amd.train_data``).  The images go to the device once (``augment.ImagePool``); with ``--augment`` every draw of an epoch
is a fresh random 256 x 256 window of a whole image, without it training runs on a fixed grid of windows, and validation always
does.  ``--augment he_staining`` / ``hed_he`` re-render the window from its image's own H&E stain basis, fitted once per
image (``ImagePool.stain_basis``); ``--augment quality`` / ``hed_he_quality`` add the Gaussian blur and the hue /
brightness / saturation jitter.  Without ``--test_data_path`` the directory is split by ``--train_fraction`` as the reference splits it.  The class count is
inferred from the labels, and the four options above work from channel 0 without ``--instances``.
"""
from __future__ import annotations

import argparse

import numpy as np

from ..log import get_logger

logger = get_logger(__name__)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train the semantic class head (1x1 or UNet) on the device with the backbone frozen")
    p.add_argument("--images", default=None, help=".npy, (N,256,256,3) uint8 or (N,3,256,256) float32 (with --labels; or --data_path)")
    p.add_argument("--labels", default=None, help=".npy, (N,256,256) integer class maps, -100 = not annotated")
    p.add_argument("--data_path", default=None,
                   help="directory with images.npy ((H,W,3) images of any size) and labels.npy ((H,W,2): instance, class), the "
                        "reference's layout; instead of --images / --labels / --instances")
    p.add_argument("--test_data_path", default=None, help="validation directory of the same layout (with --data_path)")
    p.add_argument("--train_fraction", type=float, default=0.8,
                   help="with --data_path and no --test_data_path: the share of the images that trains, the rest validates; 1 = no validation")
    p.add_argument("--subsample_fraction", type=float, default=None, help="with --data_path: train from a random share of the images")
    p.add_argument("--test_images", default=None)
    p.add_argument("--test_labels", default=None)
    p.add_argument("--pretrained_model", required=True, help="checkpoint (state dict) to adapt")
    p.add_argument("--nclasses", type=int, default=None, help="class count of a NEW head when the checkpoint has none")
    p.add_argument("--n_epochs", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--learning_rate", type=float, default=5e-5)
    p.add_argument("--weight_decay", type=float, default=0.1)
    cw = p.add_mutually_exclusive_group()
    cw.add_argument("--class_weights", type=float, nargs="+", default=None)
    cw.add_argument("--auto_class_weights", action="store_true",
                    help="class weights from the training set, sqrt(median count / count) as the reference computes them by "
                         "default (there --no_class_weights switches them off; here they are opt-in); needs --instances")
    p.add_argument("--nimg_per_epoch", type=int, default=None)
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--cache_features", action=argparse.BooleanOptionalAction, default=True,
                   help="run the frozen backbone once per crop and train from the cached neck features")
    p.add_argument("--augment", default=None, choices=["hed_only", "he_staining", "hed_he", "quality", "hed_he_quality", "geometry", "enhanced"],
                   help="augment every training batch on the device: hed_only = stain jitter + flip / rotation / scale / crop, "
                        "he_staining = H&E stain-matrix perturbation + the same geometry, hed_he = per image one of the two colour "
                        "transforms (the colour stage of enhanced) + geometry, quality = Gaussian blur + hue / brightness / "
                        "saturation jitter + geometry, hed_he_quality = hed_he followed by quality (the reference's whole enhanced "
                        "pipeline; the name enhanced itself is not enabled), geometry = the geometry alone")
    p.add_argument("--scale_range", type=float, default=0.5, help="random scale in [1 - r/2, 1 + r/2] (with --augment)")
    p.add_argument("--augment_label_fill", type=int, default=0,
                   help="class of pixels the warp takes from outside the crop: 0 = background as in the reference, -100 = not annotated")
    p.add_argument("--instances", default=None, help=".npy, (N,256,256) integer instance maps aligned with --labels (0 = background)")
    p.add_argument("--test_instances", default=None, help=".npy, instance maps of the validation set (its diameter range is logged)")
    p.add_argument("--instances_from_labels", action="store_true",
                   help="semantic-only sets: derive the instance maps on the device from --labels (and --test_labels) as the connected "
                        "regions of one class, the reference's recipe for such sets; then everything that needs --instances works.  "
                        "Touching cells of one class become one instance.  Not with --instances, --test_instances or --data_path")
    p.add_argument("--instance_connectivity", type=int, default=None, choices=[4, 8],
                   help="neighbourhood of --instances_from_labels: 4 = edges (the default, ndimage.label's in the reference's recipe), "
                        "8 = corners too")
    p.add_argument("--split_touching_cells", action="store_true",
                   help="with --instances_from_labels: cut regions that hold several touching cells at the peaks of their distance "
                        "map, every pixel to the nearest peak of its own region (straight cuts, not a flooding watershed)")
    p.add_argument("--split_min_distance", type=int, default=None,
                   help="--split_touching_cells: two peaks of one region closer than this many pixels (Chebyshev) are one cell (default 5)")
    p.add_argument("--split_min_radius", type=int, default=None,
                   help="--split_touching_cells: a peak counts only this many pixels or more inside its region (default 2)")
    p.add_argument("--oversampling_method", default="none", choices=["none", "custom"],
                   help="custom = draw every epoch with probabilities that favour crops with rare-class instances (the reference's "
                        "default; here the default is none, a plain permutation); needs --instances")
    p.add_argument("--oversampling_power", type=float, default=1.0, help="exponent of the oversampling weights")
    p.add_argument("--rescale", action="store_true",
                   help="divide the random scale of the augmentation by (cell diameter of the crop / --diam_mean); needs --instances "
                        "and --augment")
    p.add_argument("--diam_mean", type=float, default=30.0)
    p.add_argument("--min_train_masks", type=int, default=0,
                   help="drop training crops with fewer masks (the reference's default is 5; here 0 keeps every crop); needs --instances")
    p.add_argument("--feature_transformation_structure", type=int, nargs="+", default=None,
                   help="channels per level of a UNet class head (the reference's flag): a checkpoint that has such a head trains it "
                        "without this flag; given, a checkpoint without one gets a freshly initialised UNet head on its backbone "
                        "(with --nclasses when it has no classes); at most 4 levels")
    p.add_argument("--train_flow_head", action="store_true",
                   help="train the flow head (out, the flow / cell-probability logits) next to the class head, from the instance "
                        "maps: the reference's --freeze backbone neck; needs --instances or --data_path")
    p.add_argument("--train_neck", action="store_true",
                   help="train the neck (encoder.neck.*: 1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d) next to the class head, from "
                        "cached backbone rows: the reference's --freeze backbone segmentation_head; with --train_flow_head its "
                        "--freeze backbone; not with a UNet class head")
    p.add_argument("--train_blocks", type=int, default=0, metavar="K",
                   help="train the last K transformer blocks (encoder.blocks.*) next to the neck and the class head, from the cached "
                        "input rows of block depth - K; turns --train_neck on; not with a UNet class head.  --train_blocks 24 "
                        "--train_flow_head is what the reference trains without --freeze, except for the patch embedding and the "
                        "position table, which stay fixed unless --train_embed is given")
    p.add_argument("--grad_precision", default="fp32", choices=["fp32", "bf16"],
                   help="with --train_blocks: bf16 runs the matrix products of the blocks' backward on bf16 operands with float32 "
                        "accumulation (several times faster; gradients differ from the float32 backward by the operand rounding); "
                        "needs --precision bf16.  The default fp32 is the exact float32 backward")
    p.add_argument("--attn_grad_precision", default="fp32", choices=["fp32", "bf16"],
                   help="with --grad_precision bf16: bf16 runs the attention backward of the trained blocks on bf16 operands as well "
                        "(dO, P and dS' rounded once, float32 accumulation).  The default fp32 keeps it in float32")
    p.add_argument("--train_embed", action="store_true",
                   help="train the patch embedding (encoder.patch_embed.proj.*) and the position table (encoder.pos_embed) too: full "
                        "fine-tuning.  Needs --train_blocks equal to the checkpoint's depth (24 for ViT-L), because the gradient reaches "
                        "the embedding only through every block; not with a UNet class head.  The cache then holds patch rows (384 KB per "
                        "crop in bf16) and every step runs the whole network.  With --train_flow_head this is what the reference trains "
                        "without --freeze.  --grad_precision bf16 also runs the embedding's weight gradient on bf16 operands")
    p.add_argument("--layer_drop", type=float, default=0.0, metavar="RATE",
                   help="with --train_blocks: stochastic depth.  Every step drops whole trained blocks per crop, block i of the network "
                        "with probability linspace(0, RATE, depth)[i]; a dropped (block, crop) pair is not computed, forward or "
                        "backward.  The reference trains with 0.4 (rdrop); the default 0 drops nothing.  Only the trained blocks "
                        "drop (the frozen ones are cached); validation never drops; the masks are seeded from --random_seed")
    p.add_argument("--freeze", nargs="+", default=None, choices=["none", "backbone", "segmentation_head", "neck"],
                   help="the reference's spelling of the same choice: 'backbone neck' = --train_flow_head, 'backbone "
                        "segmentation_head neck' = the default (class head only); nothing else is built")
    p.add_argument("--save_only_trainable_params", action="store_true")
    p.add_argument("--random_seed", type=int, default=42)
    p.add_argument("--save_path", required=True)
    p.add_argument("--model_name", required=True)
    p.add_argument("--device", default="cuda:0")
    return p


def flow_head_from_freeze(freeze, train_flow_head: bool) -> bool:
    """Whether the flow head trains, from ``--freeze`` (the reference's flag, run_training.py:92-98) and ``--train_flow_head``.
    Raises ``SystemExit`` naming what is not built for every other combination."""
    if freeze is None:
        return bool(train_flow_head)
    parts = set(freeze)
    if "none" in parts and len(parts) > 1:
        raise SystemExit("--freeze none stands alone")
    missing = [name for name in ("backbone", "neck") if name not in parts]
    if missing:
        what = " and ".join("training the " + m for m in missing)
        raise SystemExit(f"--freeze {' '.join(freeze)}: {what} is not built; 'backbone neck' (both heads train) and 'backbone "
                         "segmentation_head neck' (the class head trains) are.  The neck trains with --train_neck (and "
                         "--train_flow_head for the flow head) in place of --freeze")
    if "segmentation_head" in parts:
        if train_flow_head:
            raise SystemExit("--train_flow_head contradicts --freeze ... segmentation_head ...: give one or the other")
        return False
    return True


def checkpoint_depth(path) -> int | None:
    """The number of transformer blocks of the checkpoint at ``path`` (its ``encoder.blocks.N.`` keys, read through a memory map), or
    None when there is no such file or no such key: whatever is wrong with it is then reported where the checkpoint is loaded."""
    import os
    import re
    if path is None or not os.path.isfile(path):
        return None
    import warnings
    import torch
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sd = torch.load(path, map_location="cpu", weights_only=True, mmap=True)
    except Exception:
        return None
    idx = [int(m.group(1)) for m in (re.match(r"(?:module\.)?encoder\.blocks\.(\d+)\.", k) for k in sd) if m]
    return max(idx) + 1 if idx else None


def check_args(args) -> None:
    """The combinations the parser cannot express; raises ``SystemExit`` with the reason."""
    args.train_neck = bool(getattr(args, "train_neck", False))
    args.train_blocks = int(getattr(args, "train_blocks", 0) or 0)
    if args.train_blocks < 0:
        raise SystemExit("--train_blocks: a count of blocks, 0 for none")
    args.grad_precision = getattr(args, "grad_precision", None) or "fp32"
    if args.grad_precision == "bf16":
        if not args.train_blocks:
            raise SystemExit("--grad_precision bf16 goes with --train_blocks K: it is the backward of the trained transformer blocks "
                             "(the neck's and the heads' gradients stay float32)")
        precision = getattr(args, "precision", "bf16")
        if precision == "fp16":
            raise SystemExit("--grad_precision bf16 needs --precision bf16: fp16 gradients would need loss scaling, which is not built")
        if precision != "bf16":
            raise SystemExit(f"--grad_precision bf16 needs --precision bf16: a {precision} network has no half-precision operands")
    args.attn_grad_precision = getattr(args, "attn_grad_precision", None) or "fp32"
    if args.attn_grad_precision == "bf16" and args.grad_precision != "bf16":
        raise SystemExit("--attn_grad_precision bf16 needs --grad_precision bf16: it is the last float32 product of the bf16 backward of "
                         "the trained blocks, not a mode of the float32 backward")
    args.layer_drop = float(getattr(args, "layer_drop", 0.0) or 0.0)
    if not 0.0 <= args.layer_drop < 1.0:
        raise SystemExit(f"--layer_drop: a rate in [0, 1), not {args.layer_drop} (the reference's rdrop is 0.4)")
    if args.layer_drop > 0 and not args.train_blocks:
        raise SystemExit("--layer_drop goes with --train_blocks K: it drops trained transformer blocks per crop (the frozen blocks run "
                         "once, into the cache, and stay deterministic)")
    args.train_embed = bool(getattr(args, "train_embed", False))
    if args.train_embed:
        if getattr(args, "feature_transformation_structure", None) is not None:
            raise SystemExit("--train_embed: the patch embedding does not train under a UNet class head (its backward gives the neck "
                             "output no gradient, so none reaches the blocks or the embedding)")
        if not args.train_blocks:
            raise SystemExit("--train_embed needs --train_blocks equal to the checkpoint's depth (24 for ViT-L): the gradient reaches "
                             "the patch embedding only through every block")
        depth = checkpoint_depth(getattr(args, "pretrained_model", None))
        if depth is not None and args.train_blocks != depth:
            raise SystemExit(f"--train_embed needs --train_blocks {depth}, the checkpoint's depth, not --train_blocks {args.train_blocks}: "
                             "the gradient reaches the patch embedding only through every block")
    if args.train_blocks:
        if getattr(args, "feature_transformation_structure", None) is not None:
            raise SystemExit("--train_blocks: the blocks do not train under a UNet class head (its backward gives the neck output no "
                             "gradient, so none reaches the blocks)")
        if "neck" in (getattr(args, "freeze", None) or ()):
            raise SystemExit("--train_blocks contradicts --freeze ... neck ...: the blocks train through the neck, which then trains too; "
                             "give one or the other")
        if not args.train_neck:
            get_logger("classpose_amd.train_head").info(">>> --train_blocks %d turns --train_neck on: the blocks' gradient comes through the neck",
                                                        args.train_blocks)
        args.train_neck = True
    if args.train_neck and "neck" in (getattr(args, "freeze", None) or ()):
        raise SystemExit("--train_neck contradicts --freeze ... neck ...: give one or the other")
    if args.train_neck and getattr(args, "feature_transformation_structure", None) is not None:
        raise SystemExit("--train_neck: the neck does not train under a UNet class head (its backward gives the neck output no gradient)")
    args.train_flow_head = flow_head_from_freeze(getattr(args, "freeze", None), getattr(args, "train_flow_head", False))
    args.instances_from_labels = derive = bool(getattr(args, "instances_from_labels", False))
    args.instance_connectivity = getattr(args, "instance_connectivity", None)
    if derive:
        clash = [f for f, v in (("--instances", args.instances), ("--test_instances", args.test_instances),
                                ("--data_path", args.data_path)) if v is not None]
        if clash:
            raise SystemExit(f"--instances_from_labels derives the instance maps from --labels: not with {', '.join(clash)}"
                             + (" (channel 0 of its labels already carries instances)" if "--data_path" in clash else ""))
    elif args.instance_connectivity is not None:
        raise SystemExit("--instance_connectivity goes with --instances_from_labels")
    args.split_touching_cells = split = bool(getattr(args, "split_touching_cells", False))
    args.split_min_distance = getattr(args, "split_min_distance", None)
    args.split_min_radius = getattr(args, "split_min_radius", None)
    if split and not derive:
        raise SystemExit("--split_touching_cells goes with --instances_from_labels")
    for flag, value, limit in (("--split_min_distance", args.split_min_distance, "SPLIT_MAX_MIN_DISTANCE"),
                               ("--split_min_radius", args.split_min_radius, "SPLIT_MAX_MIN_RADIUS")):
        if value is None:
            continue
        if not split:
            raise SystemExit(f"{flag} goes with --instances_from_labels --split_touching_cells")
        from .. import ops
        if not 1 <= value <= getattr(ops, limit):
            raise SystemExit(f"{flag}: 1 to {getattr(ops, limit)} pixels, not {value}")
    if args.train_flow_head and args.data_path is None and args.instances is None and not derive:
        raise SystemExit("--train_flow_head (--freeze backbone neck): needs --instances or --data_path, or --instances_from_labels")
    if args.train_flow_head and args.data_path is None and args.test_images is not None and args.test_instances is None and not derive:
        raise SystemExit("--train_flow_head with a validation set: needs --test_instances or --instances_from_labels")
    fts = getattr(args, "feature_transformation_structure", None)
    if fts is not None and (len(fts) > 4 or min(fts) < 1):
        raise SystemExit("--feature_transformation_structure: 1 to 4 positive channel counts (32 x 32 tokens halve once per level "
                         "and once more in the bottleneck)")
    if args.data_path is not None:
        given = [f for f, v in (("--images", args.images), ("--labels", args.labels), ("--instances", args.instances),
                                ("--test_images", args.test_images), ("--test_labels", args.test_labels),
                                ("--test_instances", args.test_instances)) if v is not None]
        if given:
            raise SystemExit(f"--data_path replaces {', '.join(given)}: give one or the other")
        if not 0.0 < args.train_fraction <= 1.0:
            raise SystemExit("--train_fraction must lie in (0, 1]")
        if args.subsample_fraction is not None and not 0.0 < args.subsample_fraction <= 1.0:
            raise SystemExit("--subsample_fraction must lie in (0, 1]")
        if args.rescale and args.augment is None:
            raise SystemExit("--rescale divides the random scale of the augmentation: it needs --augment")
        return
    if args.images is None or args.labels is None:
        raise SystemExit("give --images and --labels, or --data_path")
    if args.test_data_path is not None or args.subsample_fraction is not None:
        raise SystemExit("--test_data_path and --subsample_fraction go with --data_path")
    if (args.test_images is None) != (args.test_labels is None):
        raise SystemExit("--test_images and --test_labels go together")
    needs = [flag for flag, on in (("--auto_class_weights", args.auto_class_weights),
                                   ("--oversampling_method custom", args.oversampling_method != "none"),
                                   ("--rescale", args.rescale), ("--min_train_masks", args.min_train_masks > 0),
                                   ("--test_instances", args.test_instances is not None)) if on]
    if needs and args.instances is None and not derive:
        raise SystemExit(f"{', '.join(needs)}: needs --instances or --instances_from_labels")
    if args.test_instances is not None and args.test_labels is None:
        raise SystemExit("--test_instances needs --test_images and --test_labels")
    if args.rescale and args.augment is None:
        raise SystemExit("--rescale divides the random scale of the augmentation: it needs --augment")


def _load_instances(path, labels, what: str) -> np.ndarray:
    inst = np.load(path)
    if inst.shape != labels.shape or not np.issubdtype(inst.dtype, np.integer):
        raise SystemExit(f"{what}: expected integer instance maps {labels.shape}, got {inst.shape} {inst.dtype}")
    return inst


def _derive_instances(labels, args, what: str):
    """``--instances_from_labels``: the connected regions of one class, labelled on the device (dataset_stats.instances_from_classes);
    the int32 maps stay there for the statistics."""
    from .. import dataset_stats
    if labels.ndim != 3 or not np.issubdtype(labels.dtype, np.integer):
        raise SystemExit(f"{what}: --instances_from_labels expects (N, H, W) integer class maps, got {labels.shape} {labels.dtype}")
    connectivity = 4 if args.instance_connectivity is None else args.instance_connectivity
    inst, counts = dataset_stats.instances_from_classes(labels, connectivity, device=args.device)
    logger.info(f"{what}: derived {int(counts.sum())} instances from {len(labels)} class maps ({connectivity}-connected regions of one "
                f"class; {int(counts.min()) if len(counts) else 0} to {int(counts.max()) if len(counts) else 0} per map)")
    if args.split_touching_cells:
        md = 5 if args.split_min_distance is None else args.split_min_distance
        mr = 2 if args.split_min_radius is None else args.split_min_radius
        cut, _ = dataset_stats.instances_from_classes(labels, connectivity, device=args.device, split_touching=True, min_distance=md,
                                                      min_radius=mr)
        n_comp, n_split, n_inst = dataset_stats.split_summary(inst, cut)
        logger.info(f"{what}: --split_touching_cells cut {n_split} of {n_comp} components into pieces, {n_inst} instances in all "
                    f"(min_distance {md}, min_radius {mr})")
        inst = cut
    return inst


def _host_maps(instances):
    """instance maps for the flow targets, which renumber ids on the host: derived maps come from the device"""
    return instances.cpu().numpy() if hasattr(instances, "cpu") else instances


def _trainer_of(args, make_trainer, nclasses):
    """The trainer the arguments ask for; a block count the checkpoint does not have ends the run with the reason."""
    try:
        trainer = make_trainer(args.pretrained_model, nclasses=nclasses, device=args.device, precision=args.precision,
                               feature_transformation_structure=args.feature_transformation_structure,
                               class_weights=args.class_weights, weight_decay=args.weight_decay, train_flow_head=args.train_flow_head,
                               train_neck=args.train_neck, train_blocks=args.train_blocks,
                               **({"grad_precision": "bf16"} if getattr(args, "grad_precision", "fp32") == "bf16" else {}),
                               **({"attn_grad_precision": "bf16"} if getattr(args, "attn_grad_precision", "fp32") == "bf16" else {}),
                               **({"train_embed": True} if getattr(args, "train_embed", False) else {}),
                               **({"layer_drop": args.layer_drop, "layer_drop_seed": args.random_seed} if getattr(args, "layer_drop", 0.0) > 0 else {}))
    except (ValueError, NotImplementedError) as e:
        if getattr(args, "train_embed", False) and "train_embed" in str(e):
            raise SystemExit(f"--train_embed: {e}")
        if args.train_blocks and "train_blocks" in str(e):
            raise SystemExit(f"--train_blocks {args.train_blocks}: {e}")
        raise
    if getattr(args, "layer_drop", 0.0) > 0:
        from ..train import layer_drop_probs
        depth, K = trainer.weights.depth, trainer.train_blocks
        probs = layer_drop_probs(depth, args.layer_drop)[depth - K:]
        logger.info(f">>> --layer_drop {args.layer_drop:g}: blocks {depth - K} to {depth - 1} of {depth} are dropped per crop with "
                    f"probabilities {', '.join(f'{v:.4f}' for v in probs)} ({probs.mean():.1%} of the trained (block, crop) pairs on "
                    f"average), masks seeded with {args.random_seed}" + ("" if K == depth else "; the frozen blocks never drop"))
    return trainer


def main_data_path(args) -> None:
    """``--data_path``: whole annotated images of any size, from the reference's directory to a device pool."""
    from .. import augment, dataset_stats, train_data
    from ..train import make_trainer, train_class_head
    data = train_data.load_dataset(args.data_path)
    logger.info(f"{args.data_path}: {len(data)} images, inferred number of classes: {data.n_classes}")
    data = data.subset(train_data.subsample_indices(len(data), args.subsample_fraction, args.random_seed))
    if args.test_data_path is not None:
        test = train_data.load_dataset(args.test_data_path)
    else:
        tr, te = train_data.split_indices(len(data), args.train_fraction, args.random_seed)
        data, test = data.subset(tr), (None if te is None or len(te) == 0 else data.subset(te))
    logger.info(f"{len(data)} training images, {len(test) if test is not None else 0} validation images")
    nclasses = data.n_classes if args.nclasses is None else args.nclasses
    trainer = _trainer_of(args, make_trainer, nclasses)
    if data.n_classes > trainer.nclasses:
        raise SystemExit(f"the labels hold class {data.n_classes - 1} but the head has {trainer.nclasses} classes")
    train_probs = diameters = None
    if args.auto_class_weights or args.oversampling_method != "none" or args.rescale or args.min_train_masks > 0 or args.train_flow_head:
        stats = train_data.ragged_label_stats(data.instances, data.classes, trainer.nclasses, device=args.device)
        diameters = dataset_stats.clamp_diameters(stats.diameters)
        logger.info(f"diameters: {diameters.min():.2f} to {diameters.max():.2f} px, masks per image: {int(stats.n_masks.min())} to "
                    f"{int(stats.n_masks.max())}")
        if args.min_train_masks > 0:
            keep = np.nonzero(stats.n_masks >= args.min_train_masks)[0]
            if len(keep) < len(data):
                logger.warning(f"{len(data) - len(keep)} train images with number of masks less than min_train_masks "
                               f"({args.min_train_masks}), removing from train set")
                if len(keep) == 0:
                    raise SystemExit("--min_train_masks leaves no training image")
                data, diameters = data.subset(keep), diameters[keep]
                stats = dataset_stats.LabelStats(stats.class_counts, stats.instance_counts[keep], stats.n_masks[keep],
                                                 stats.diameters[keep])
        if args.auto_class_weights:
            logger.info("Computing class weights using inverse frequency with square root scaling")
            weights = dataset_stats.get_class_weights(stats.class_counts)
            logger.info(f"class weights = {weights.tolist()}")
            trainer.set_class_weights(weights)
        if args.oversampling_method == "custom":
            logger.info(f"Computing oversampling probabilities with power {args.oversampling_power}")
            train_probs = dataset_stats.compute_oversampling_probabilities(stats.class_counts, stats.instance_counts,
                                                                           args.oversampling_power)
            if not np.all(np.isfinite(train_probs)):
                raise SystemExit("--oversampling_method custom: the training set has no instance of a class above 0")
            logger.info(f"Custom oversampling - probability range: {train_probs.min():.6f} to {train_probs.max():.6f}")
    if args.train_flow_head:
        logger.info(f"computing the flow targets of {len(data)} training images" + (f" and {len(test)} validation images" if test is not None else ""))
        trainer.set_diam_labels(diameters)
    pool = augment.ImagePool(data.images, data.classes, diameters if args.rescale else None, device=args.device,
                             instances=data.instances if args.train_flow_head else None)
    test_pool = None if test is None else augment.ImagePool(test.images, test.classes, device=args.device,
                                                            instances=test.instances if args.train_flow_head else None)
    logger.info(f"image pool: {pool.nbytes / 2 ** 20:.1f} MB on the device for {len(pool)} images"
                + (" (12 of its 17 bytes per pixel are the flow targets)" if args.train_flow_head else ""))
    path, train_losses, test_losses = train_class_head(
        trainer, pool, None, test_pool, None, batch_size=args.batch_size, n_epochs=args.n_epochs,
        learning_rate=args.learning_rate, nimg_per_epoch=args.nimg_per_epoch, cache_features=args.cache_features,
        save_path=args.save_path, model_name=args.model_name, random_seed=args.random_seed,
        augment=args.augment, scale_range=args.scale_range, label_fill=args.augment_label_fill, train_probs=train_probs,
        diam_mean=args.diam_mean, rescale=args.rescale, train_flow_head=args.train_flow_head)
    if args.save_only_trainable_params:
        trainer.save(path, save_only_trainable_params=True)
    logger.info(f"final train loss {train_losses[-1]:.4f}" + (f", test loss {test_losses[-1]:.4f}" if test_pool is not None else ""))
    print(path)


def main(args) -> None:
    from .. import dataset_stats
    from ..train import make_trainer, train_class_head
    check_args(args)
    if args.data_path is not None:
        return main_data_path(args)
    images, labels = np.load(args.images), np.load(args.labels)
    test_images = np.load(args.test_images) if args.test_images else None
    test_labels = np.load(args.test_labels) if args.test_labels else None
    trainer = _trainer_of(args, make_trainer, args.nclasses)
    train_probs = diameters = instances = test_instances = None
    if args.instances_from_labels:
        instances = _derive_instances(labels, args, "--labels")
        if test_labels is not None:
            test_instances = _derive_instances(test_labels, args, "--test_labels")
        if not args.split_touching_cells:
            logger.warning("--instances_from_labels: touching cells of one class merge into one instance")
    if instances is not None or args.instances is not None:
        if instances is None:
            instances = _load_instances(args.instances, labels, "--instances")
        stats = dataset_stats.label_stats(instances, labels, trainer.nclasses, device=args.device)
        diameters = dataset_stats.clamp_diameters(stats.diameters)                # train_utils.py:268
        logger.info(f"diameters: {diameters.min():.2f} to {diameters.max():.2f} px, masks per image: {int(stats.n_masks.min())} to "
                    f"{int(stats.n_masks.max())}")
        if args.test_instances is not None or test_instances is not None:
            if test_instances is None:
                test_instances = _load_instances(args.test_instances, test_labels, "--test_instances")
            tstats = dataset_stats.label_stats(test_instances, test_labels, trainer.nclasses, device=args.device)
            tdiam = dataset_stats.clamp_diameters(tstats.diameters)
            logger.info(f"test diameters: {tdiam.min():.2f} to {tdiam.max():.2f} px")
        if args.min_train_masks > 0:                                               # train_utils.py:288-308
            keep = np.nonzero(stats.n_masks >= args.min_train_masks)[0]
            nremove = len(images) - len(keep)
            if nremove > 0:
                logger.warning(f"{nremove} train images with number of masks less than min_train_masks ({args.min_train_masks}), "
                               "removing from train set")
                if len(keep) == 0:
                    raise SystemExit("--min_train_masks leaves no training image")
                images, labels, diameters, instances = images[keep], labels[keep], diameters[keep], instances[keep]
                stats = dataset_stats.LabelStats(stats.class_counts, stats.instance_counts[keep], stats.n_masks[keep],
                                                 stats.diameters[keep])
        # like the reference, weights and probabilities use the class counts of the whole set as loaded (run_training.py computes
        # them before process_and_build_dataset removes images); the probabilities of removed images leave with them
        if args.auto_class_weights:
            logger.info("Computing class weights using inverse frequency with square root scaling")
            weights = dataset_stats.get_class_weights(stats.class_counts)
            logger.info(f"class weights = {weights.tolist()}")
            trainer.set_class_weights(weights)
        if args.oversampling_method == "custom":
            logger.info(f"Computing oversampling probabilities with power {args.oversampling_power}")
            train_probs = dataset_stats.compute_oversampling_probabilities(stats.class_counts, stats.instance_counts,
                                                                           args.oversampling_power)
            if not np.all(np.isfinite(train_probs)):
                raise SystemExit("--oversampling_method custom: the training set has no instance of a class above 0")
            logger.info(f"Custom oversampling - probability range: {train_probs.min():.6f} to {train_probs.max():.6f}")
    if args.train_flow_head:
        trainer.set_diam_labels(diameters)
    path, train_losses, test_losses = train_class_head(
        trainer, images, labels, test_images, test_labels, batch_size=args.batch_size, n_epochs=args.n_epochs,
        learning_rate=args.learning_rate, nimg_per_epoch=args.nimg_per_epoch, cache_features=args.cache_features,
        save_path=args.save_path, model_name=args.model_name, random_seed=args.random_seed,
        augment=args.augment, scale_range=args.scale_range, label_fill=args.augment_label_fill, train_probs=train_probs,
        diameters=diameters if args.rescale else None, diam_mean=args.diam_mean, rescale=args.rescale,
        train_flow_head=args.train_flow_head, instances=_host_maps(instances) if args.train_flow_head else None,
        test_instances=_host_maps(test_instances) if args.train_flow_head else None)
    if args.save_only_trainable_params:
        trainer.save(path, save_only_trainable_params=True)
    logger.info(f"final train loss {train_losses[-1]:.4f}" + (f", test loss {test_losses[-1]:.4f}" if test_images is not None else ""))
    print(path)


if __name__ == "__main__":
    main(build_parser().parse_args())
