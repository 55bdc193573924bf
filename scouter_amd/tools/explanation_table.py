"""The explanation table of the SCOUTER paper over a validation set: one row per explanation family, one column per score, every
cell a mean over --table_images images of the validation loader (seeded synthetic ones under --synthetic_data true).

The parser is the single-image tool's (scouter_amd/test.py: every family flag and option keeps its name and default) plus five
options of its own, and the families are that tool's table plus one row, `fccam` -- CAM of the --use_slot false baseline
(tools/attribution.py fccam).  Per batch: one eval forward gives the predictions; every chosen family explains each image's
target class (--table_target pred | label) in one batched call with a LongTensor of classes; the float map is drawn to bytes at
the image size (kernels.cam_maps for a coarse map, kernels.heat_maps for one already at image size, floored at
--grad_min_level) and scored:

    --localization true   area size, precision and pointing game of the byte map (tools/attribution.py localization) against the
                          boxes of the batch ("boxes" / "n_boxes" entries), of --boxes_file, or -- under synthetic data with no
                          file -- one seeded box per image; for `slot` also `ratio`, the reference's own attention_ratio
                          (test.py:40-44) of the byte slot map at its native grid (tools/attribution.py slot_maps)
    --causal true         deletion and insertion (causal_metrics, --causal_step, batches of --rise_batch)
    --infidelity true     infidelity (infidelity; grad, ig and smoothgrad with their full attribution, the others with their map)

--sensitivity is refused: sensitivity_max explains perturbed rows that carry no class of their own.  Per-image values stay on the
device in float64; nothing is read on the host inside the loop over batches (the class tensor aside, as in every family), one
transfer at the end, means in float64 NumPy in image order.  Precision and pointing are averaged over the images that have a box
and a non-empty map.  One line per family, in table order, holding only the columns asked for, then the accuracy:

    table <family>: images <n> area <a> [ratio <r>] precision <p> pointing <g> boxed <m> empty <e> deletion <d> insertion <i> infidelity <raw> <normalized>
    table accuracy <acc> images <n>

--boxes_file holds lines `<name> x0 y0 x1 y1` in fractions of the image side, matched to the batch's `names`; several lines of a
name give several boxes; a fraction becomes pixels as floor(f0 * S) and ceil(f1 * S), so the file does not depend on the image
size.  CUB's bounding_boxes.txt (`<id> x y width height` in pixels of the native image) becomes such a file by dividing x and
x + width by the image's width and y and y + height by its height, under the name the loader gives the image.

    python -m scouter_amd.tools.explanation_table --model resnest26d --dataset ImageNet --channel 2048 --num_classes 10 \
        --slots_per_class 1 --to_k_layer 3 --power 2 --use_slot true --pre_trained false --img_size 224 --batch_size 16 \
        --table_images 64 --localization true --causal true --infidelity true --cam true --rise true [--boxes_file boxes.txt]"""
import argparse
import collections
import math

import numpy as np
import torch

from .. import test as T
from ..train import _flag

# the single-image tool's families and the one that exists for the baseline only
FAMILIES = T.FAMILIES + (T.Family("fccam", "CAM heat map of the FC baseline", maps="fccam_maps", explain="fccam"),)
_ROWS = {row.name: row for row in FAMILIES + T.SCORES}
# the per-image columns in printed order; `infidelity` prints two values
COLUMNS = ("area", "ratio", "precision", "pointing", "boxed", "empty", "deletion", "insertion", "infidelity_raw",
           "infidelity_normalized")
MAX_BOXES = 32                                                   # (kernels.map_localization)

ExplanationTable = collections.namedtuple("ExplanationTable", "rows predictions correct")
ExplanationTable.__doc__ = """The result of `explanation_table`: rows {family: {column: float64 array [n]}} (the columns of COLUMNS
that were asked for, one value per image in loader order), predictions int64 [n] and correct bool [n] (NumPy, on the host)."""


# ------------------------------------------------------------------------------------------------ the command line
def get_table_parser():
    """the single-image tool's parser plus this tool's five options"""
    parser = argparse.ArgumentParser("explanation table over a validation set", parents=[T.get_test_parser()], add_help=False)
    parser.add_argument("--table_images", default=64, type=int, help="images scored, in the validation loader's order")
    parser.add_argument("--table_target", default="pred", choices=("pred", "label"),
                        help="the class every family explains: the prediction or the label")
    parser.add_argument("--fccam", default=False, type=_flag, help="true: the row of CAM (the --use_slot false baseline only)")
    parser.add_argument("--localization", default=False, type=_flag,
                        help="true: area size, precision and pointing game of every family's byte map")
    parser.add_argument("--boxes_file", default="", help="lines `<name> x0 y0 x1 y1` in fractions of the image side")
    return parser


def chosen_families(args, families=FAMILIES):
    """the names of the families a parsed command line asks for, in table order: slot with --use_slot true, grad with --grad,
    every other one by its own flag.  families: this tool's table, or one that extends it (tools/surrogate.py)"""
    unflagged = {"slot": bool(args.use_slot), "grad": bool(args.grad)}
    return [f.name for f in families if (getattr(args, f.name, False) if f.flag else unflagged[f.name])]


def check_request(families, use_slot, sensitivity=False, rows=_ROWS):
    """refuses, before any work, what the table cannot hold (rows: the table the names are looked up in)"""
    if sensitivity:
        raise ValueError("--sensitivity is not a column of the table: sensitivity_max explains perturbed rows that carry no class "
                         "of their own; score one image with `python -m scouter_amd.test --sensitivity true`")
    for name in families:
        T._row(name, rows)
    if "fccam" in families and use_slot:
        raise ValueError("fccam: CAM reads the fc layer of the --use_slot false baseline; the slot model has none (use --cam, "
                         "Grad-CAM, for it)")
    if "slot" in families and not use_slot:
        raise ValueError("slot: the --use_slot false baseline has no slot maps")


# ------------------------------------------------------------------------------------------------ the boxes
def read_boxes_file(path):
    """{name: [(x0, y0, x1, y1), ...]} in fractions of the image side from lines `<name> x0 y0 x1 y1`; blank lines are skipped,
    anything else that does not read as a name and four numbers is a ValueError naming the line"""
    table = {}
    with open(path) as f:
        for number, line in enumerate(f, 1):
            words = line.split()
            if not words:
                continue
            try:
                if len(words) != 5:
                    raise ValueError
                box = tuple(float(v) for v in words[1:])
                if not all(math.isfinite(v) for v in box):
                    raise ValueError
            except ValueError:
                raise ValueError("%s line %d: expected `<name> x0 y0 x1 y1`, got %r" % (path, number, line.rstrip("\n"))) from None
            table.setdefault(words[0], []).append(box)
    return table


def box_pixels(box, H, W):
    """fractions (x0, y0, x1, y1) of the image side -> the half-open pixel box (floor(x0 W), floor(y0 H), ceil(x1 W), ceil(y1 H))"""
    x0, y0, x1, y1 = box
    return (int(math.floor(x0 * W)), int(math.floor(y0 * H)), int(math.ceil(x1 * W)), int(math.ceil(y1 * H)))


def synthetic_box(index, H, W):
    """the one seeded box of synthetic image `index` (its position in loader order), in pixels: numpy.random.default_rng(index)
    draws a corner in the upper left half and a side of a quarter to a half of the image"""
    u = np.random.default_rng(int(index)).random(4)
    return box_pixels((0.5 * u[0], 0.5 * u[1], 0.5 * u[0] + 0.25 + 0.25 * u[2], 0.5 * u[1] + 0.25 + 0.25 * u[3]), H, W)


def batch_boxes(per_image):
    """a list of lists of pixel boxes, one list per image -> (boxes int32 [B, max(1, most boxes), 4], n_boxes int32 [B]), NumPy"""
    most = max([len(b) for b in per_image] + [1])
    if most > MAX_BOXES:
        raise ValueError("an image has %d boxes (at most %d)" % (most, MAX_BOXES))
    boxes = np.zeros((len(per_image), most, 4), dtype=np.int32)
    for i, image_boxes in enumerate(per_image):
        for j, b in enumerate(image_boxes):
            boxes[i, j] = b
    return boxes, np.array([len(b) for b in per_image], dtype=np.int32)


def named_boxes(names, table, H, W):
    """the boxes of the images called `names` from a read_boxes_file table, in pixels of an H x W image; an unknown name has none"""
    return batch_boxes([[box_pixels(b, H, W) for b in table.get(str(name), ())] for name in names])


def table_batches(args, loader, boxes_table=None):
    """the first --table_images images of `loader` as the batches `explanation_table` reads: {"image": fp32 [B, C, H, W] on the
    device (through the loader's GPU transform where it is raw), "label", and -- under --localization -- "boxes" / "n_boxes"}: the
    loader's own where it gives them, else those of `boxes_table` by the batch's names, else (synthetic data) one seeded box each"""
    transform, left, index = getattr(loader, "gpu_transform", None), int(args.table_images), 0
    for batch in loader:
        if left <= 0:
            break
        images = batch["image"]
        images = images.to(args.device, dtype=torch.float32) if torch.is_tensor(images) else transform(images, args.device)
        n = min(left, int(images.shape[0]))
        out = {"image": images[:n].contiguous(), "label": batch["label"][:n].to(args.device, dtype=torch.int64)}
        H, W = images.shape[-2:]
        if args.localization:
            if "boxes" in batch:
                boxes, n_boxes = batch["boxes"][:n], batch["n_boxes"][:n]
            elif boxes_table is not None:
                boxes, n_boxes = named_boxes(list(batch.get("names", [""] * n))[:n], boxes_table, H, W)
            elif getattr(args, "synthetic_data", True):
                boxes, n_boxes = batch_boxes([[synthetic_box(index + i, H, W)] for i in range(n)])
            else:
                boxes = n_boxes = None
            if boxes is not None:
                out["boxes"] = torch.as_tensor(boxes, dtype=torch.int32).to(args.device).contiguous()
                out["n_boxes"] = torch.as_tensor(n_boxes, dtype=torch.int32).to(args.device).contiguous()
        yield out
        left, index = left - n, index + n


# ------------------------------------------------------------------------------------------------ the table
def byte_maps(maps, H, W, min_level=0.0):
    """float maps [B, K, h, w] -> uint8 [B, K, H, W]: kernels.heat_maps when they are at the image's size already (any size),
    kernels.cam_maps otherwise (its source lives in LDS: at most 32768 pixels)"""
    from .. import kernels as K
    maps = maps.detach().float().contiguous()
    return K.heat_maps(maps, min_level) if tuple(maps.shape[-2:]) == (H, W) else K.cam_maps(maps, H, W, min_level)


def _pick(maps, target):
    """column target[b] of maps [B, C, ...] -> [B, 1, ...], on the device"""
    return maps[torch.arange(maps.shape[0], device=maps.device), target].unsqueeze(1).contiguous()


def explanation_table(args, model, batches, families, rows=_ROWS):
    """Scores the families named in `families` (rows of FAMILIES -- or of `rows`, a table that extends this tool's -- any order
    given is kept) over `batches` -> ExplanationTable.

    batches: an iterable of {"image": fp32 [B, C, H, W] on the device, "label": int64 [B], and optionally "boxes" int32
    [B, nb, 4] / "n_boxes" int32 [B] on the device, pixel boxes of the image's own grid}.  `args` is a namespace of the table
    tool's parser; an option it lacks takes the parser's default (localization, causal and infidelity: off; table_target: pred).
    Per batch one eval forward predicts, every family explains each image's target class, and the scores asked for are taken as
    the module docstring says.  Every per-image value is kept on the device as float64 and nothing is read on the host inside
    the loop (the families bring the class tensor over, as everywhere); one transfer at the end."""
    from . import attribution as A
    families = list(families)
    check_request(families, bool(model.use_slot), bool(getattr(args, "sensitivity", False)), rows)
    want_loc, want_causal = bool(getattr(args, "localization", False)), bool(getattr(args, "causal", False))
    want_inf, by_label = bool(getattr(args, "infidelity", False)), getattr(args, "table_target", "pred") == "label"
    min_level = float(getattr(args, "grad_min_level", 0.0))
    causal_kwargs = dict(T.option_kwargs(args, "causal"), batch=T.option_kwargs(args, "rise")["batch"])
    infidelity_kwargs = T.option_kwargs(args, "infidelity")
    names = ["prediction", "correct"]                            # one name per column of the device record, then per family
    for name in families:
        cols = (["area"] + (["ratio"] if name == "slot" else []) + ["precision", "pointing", "boxed", "empty"]) * want_loc + \
            ["deletion", "insertion"] * want_causal + ["infidelity_raw", "infidelity_normalized"] * want_inf
        names += [(name, c) for c in cols]
    record = []                                                  # per batch: float64 [B, len(names)] on the device
    for batch in batches:
        x, label = batch["image"], batch["label"]
        B, _, H, W = x.shape
        with A._eval_mode(model), torch.no_grad():
            pred = model(x).argmax(dim=1)
        target = label if by_label else pred
        values = {"prediction": pred.double(), "correct": (pred == label).double()}
        if "slot" in families:                                   # (before another forward replaces last_attn)
            slot_map = _pick(A.slot_saliency(model), target)
            if want_loc:
                values[("slot", "ratio")] = _pick(A.localization(A.slot_maps(model)).area, target)[:, 0]
        for name in families:
            row = T._row(name, rows)
            if row.explain is None:
                attr = fmap = slot_map
            else:
                attr = T._call(args, model, x, row, row.explain, classes=target)
                fmap = attr if row.reduce is None else row.reduce(attr)
            if want_loc:
                loc = A.localization(byte_maps(fmap, H, W, min_level), batch.get("boxes"), batch.get("n_boxes"))
                values[(name, "area")], values[(name, "precision")] = loc.area[:, 0], loc.precision[:, 0]
                values[(name, "pointing")], values[(name, "empty")] = loc.hit[:, 0], loc.empty[:, 0].double()
                values[(name, "boxed")] = loc.boxed.double()
            if want_causal:
                r = A.causal_metrics(model, x, fmap, classes=target, **causal_kwargs)
                values[(name, "deletion")], values[(name, "insertion")] = r.deletion[:, 0].double(), r.insertion[:, 0].double()
            if want_inf:
                r = A.infidelity(model, x, attr, classes=target, **infidelity_kwargs)
                values[(name, "infidelity_raw")] = r.raw[:, 0].double()
                values[(name, "infidelity_normalized")] = r.normalized[:, 0].double()
        record.append(torch.stack([values[n] for n in names], dim=1))
    if not record:
        raise ValueError("explanation_table: no batch to score")
    host = torch.cat(record, dim=0).cpu().numpy()                # the one transfer
    rows = {name: {} for name in families}
    for j, n in enumerate(names[2:], 2):
        rows[n[0]][n[1]] = host[:, j].copy()
    return ExplanationTable(rows, host[:, 0].astype(np.int64), host[:, 1] != 0.0)


def column_means(columns):
    """{column: per-image array} of one family -> {column: the printed value}: float64 NumPy means in image order; precision and
    pointing over the images with a box and a non-empty map (nan when there is none), boxed and empty as counts"""
    means = {}
    for name, v in columns.items():
        v = np.asarray(v, dtype=np.float64)
        if name in ("boxed", "empty"):
            means[name] = int(v.sum())
        elif name in ("precision", "pointing"):
            keep = (np.asarray(columns["boxed"]) != 0) & (np.asarray(columns["empty"]) == 0)
            means[name] = float(v[keep].mean()) if keep.any() else float("nan")
        else:
            means[name] = float(v.mean())
    return means


def format_row(family, columns, images=None):
    """the printed line of one family: `table <family>: images <n>` and then, in the order of COLUMNS, only the columns given
    (images: n where no column says it)"""
    means = column_means(columns)
    n = len(next(iter(columns.values()))) if columns else int(images or 0)
    words = ["table %s: images %d" % (family, n)]
    for name in COLUMNS:
        if name not in means:
            continue
        if name in ("boxed", "empty"):
            words.append("%s %d" % (name, means[name]))
        elif name == "infidelity_raw":
            words.append("infidelity %.6e" % means[name])
        elif name == "infidelity_normalized":
            words.append("%.6e" % means[name])
        else:
            words.append("%s %.6f" % (name, means[name]))
    return " ".join(words)


def run_table(args, table=FAMILIES, rows=_ROWS):
    """what main() does with a parsed command line; table / rows: this tool's families, or a table that extends them
    (tools/surrogate.py)"""
    # (BEFORE build_model: it clears args.grad, the flag of the grad row, so that the model is built as for training)
    families = chosen_families(args, table)
    check_request(families, bool(args.use_slot), bool(args.sensitivity), rows)
    if args.table_images < 1:
        raise ValueError("--table_images must be at least 1, got %d" % args.table_images)
    boxes_table = read_boxes_file(args.boxes_file) if args.boxes_file else None
    model, _ = T.build_model(args)
    from ..train import _build_loaders
    args.distributed = bool(getattr(args, "distributed", False))
    _, loader, _ = _build_loaders(args)
    result = explanation_table(args, model, table_batches(args, loader, boxes_table), families, rows)
    for name in families:
        print(format_row(name, result.rows[name], len(result.correct)))
    print("table accuracy %.6f images %d" % (float(result.correct.mean()), len(result.correct)))
    return result


def main():
    return run_table(get_table_parser().parse_args())


if __name__ == "__main__":
    main()
