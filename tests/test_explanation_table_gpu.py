"""The table tool on the device (-m gpu): one main() call on the slot model at the smallest settings that fill every column, the
library entry against direct calls of tools/attribution.py on the same batches bit for bit, a main() call on the --use_slot
false baseline with the fccam row, and the refusal of fccam on a slot model before any model is built."""
import math
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODEL = ["--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
         "--to_k_layer", "1", "--power", "1", "--pre_trained", "false", "--img_size", "64", "--synthetic_data", "true",
         "--num_workers", "0", "--table_images", "8", "--batch_size", "4"]


def _lines(text, families):
    """the `table` lines of a run as {family: {word: [values]}}, checked for their order and the accuracy line at the end"""
    lines = [ln for ln in text.splitlines() if ln.startswith("table ")]
    assert [ln.split()[1] for ln in lines] == [f + ":" for f in families] + ["accuracy"]
    assert text.splitlines()[-1] == lines[-1]
    acc = lines[-1].split()
    assert acc[:2] == ["table", "accuracy"] and 0.0 <= float(acc[2]) <= 1.0 and acc[3:] == ["images", "8"]
    rows = {}
    for ln in lines[:-1]:
        words, row, key = ln.split(), {}, None
        for word in words[2:]:
            try:
                value = float(word)
            except ValueError:
                key = word
                row[key] = []
            else:
                row[key].append(value)
        assert all(math.isfinite(v) for vs in row.values() for v in vs), ln
        rows[words[1][:-1]] = row
    return rows


def test_one_call_on_the_slot_model(tmp_path, monkeypatch, capsys):
    from scouter_amd.tools import explanation_table as X
    torch.manual_seed(5)
    monkeypatch.setattr(sys, "argv", ["explanation_table.py"] + MODEL + [
        "--use_slot", "true", "--localization", "true", "--causal", "true", "--causal_step", "2048", "--infidelity", "true",
        "--infidelity_samples", "3", "--cam", "true", "--rise", "true", "--rise_masks", "6", "--rise_batch", "4", "--grad", "true",
        "--output_dir", str(tmp_path / "none")])
    result = X.main()
    rows = _lines(capsys.readouterr().out, ["slot", "grad", "cam", "rise"])
    for name, row in rows.items():
        want = ["images", "area"] + (["ratio"] if name == "slot" else []) + ["precision", "pointing", "boxed", "empty", "deletion",
                                                                             "insertion", "infidelity"]
        assert list(row) == want, name
        assert row["images"] == [8.0] and 0.0 <= row["area"][0] <= 1.0 and len(row["infidelity"]) == 2
        assert 0.0 <= row["precision"][0] <= 1.0 and 0.0 <= row["pointing"][0] <= 1.0
        assert row["boxed"] == [8.0]                                         # synthetic data: one seeded box an image
        cols = result.rows[name]
        assert all(v.dtype == np.float64 and v.shape == (8,) for v in cols.values())
        # the printed means are the NumPy means of the per-image values
        assert "%.6f" % row["area"][0] == "%.6f" % cols["area"].mean()
        assert "%.6f" % row["deletion"][0] == "%.6f" % cols["deletion"].mean()
        assert "%.6e" % row["infidelity"][0] == "%.6e" % cols["infidelity_raw"].mean()
    assert 0.0 < rows["slot"]["ratio"][0] <= 1.0
    assert result.predictions.shape == (8,) and result.correct.shape == (8,)


def test_the_library_entry_equals_direct_calls(tmp_path):
    """slot, grad and cam over two batches of four: every per-image value of the table is the value of the direct library call on
    the same batch, bit for bit -- gradcam + cam_maps + localization, slot_saliency + cam_maps + localization, input_gradients
    with the tensor of predictions + channel mean + heat_maps + localization, slot_maps' area at the target column,
    causal_metrics of the three float maps, and infidelity of the two maps and of the full gradient"""
    from scouter_amd import kernels as K
    from scouter_amd import test as T
    from scouter_amd.tools import attribution as A
    from scouter_amd.tools import explanation_table as X
    from scouter_amd.train import _build_loaders
    torch.manual_seed(6)
    args = X.get_table_parser().parse_args(MODEL + ["--use_slot", "true", "--localization", "true", "--causal", "true",
                                                    "--causal_step", "2048", "--rise_batch", "4", "--grad_min_level", "0.1",
                                                    "--infidelity", "true", "--infidelity_samples", "3", "--cam", "true", "--output_dir", str(tmp_path / "none")])
    model, _ = T.build_model(args)
    args.distributed = False
    _, loader, _ = _build_loaders(args)
    batches = list(X.table_batches(args, loader))
    assert [tuple(b["image"].shape) for b in batches] == [(4, 1, 64, 64)] * 2
    assert all(tuple(b["boxes"].shape) == (4, 1, 4) and b["n_boxes"].tolist() == [1] * 4 for b in batches)
    assert batches[1]["boxes"][0].cpu().tolist() == [list(X.synthetic_box(4, 64, 64))]        # seeded by the image's index
    result = X.explanation_table(args, model, batches, ["slot", "grad", "cam"])
    assert list(result.rows) == ["slot", "grad", "cam"]
    columns = ("area", "precision", "pointing", "boxed", "empty", "deletion", "insertion", "infidelity_raw", "infidelity_normalized")
    want = {(name, c): [] for name in ("slot", "grad", "cam") for c in columns}
    want[("slot", "ratio")] = []
    preds = []
    for b in batches:
        x = b["image"]
        with A._eval_mode(model), torch.no_grad():
            pred = model(x).argmax(dim=1)
        preds.append(pred.cpu())
        idx = torch.arange(4, device=x.device)
        slot = A.slot_saliency(model)[idx, pred].unsqueeze(1).contiguous()
        want[("slot", "ratio")].append(A.localization(A.slot_maps(model)).area[idx, pred])
        grad = A.input_gradients(model, x, classes=pred)
        assert tuple(grad.shape) == (4, 1, 1, 64, 64)
        for name, attr in (("slot", slot), ("grad", grad), ("cam", A.gradcam(model, x, classes=pred))):
            # (grad: the full attribution is what infidelity scores; its channel mean is the map, already at the image's size)
            fmap = attr.mean(dim=2).contiguous() if name == "grad" else attr
            drawn = K.heat_maps(fmap, 0.1) if name == "grad" else K.cam_maps(fmap, 64, 64, 0.1)
            loc = A.localization(drawn, b["boxes"], b["n_boxes"])
            r = A.causal_metrics(model, x, fmap, classes=pred, step=2048, batch=4)
            f = A.infidelity(model, x, attr, classes=pred, n_samples=3, sigma=0.003, batch=50)
            for c, v in (("area", loc.area[:, 0]), ("precision", loc.precision[:, 0]), ("pointing", loc.hit[:, 0]),
                         ("boxed", loc.boxed), ("empty", loc.empty[:, 0]), ("deletion", r.deletion[:, 0]),
                         ("insertion", r.insertion[:, 0]), ("infidelity_raw", f.raw[:, 0]),
                         ("infidelity_normalized", f.normalized[:, 0])):
                want[(name, c)].append(v.double())
    assert np.array_equal(result.predictions, torch.cat(preds).numpy())
    for (name, c), parts in want.items():
        direct = torch.cat(parts).cpu().numpy()
        assert direct.dtype == np.float64 and np.array_equal(result.rows[name][c], direct), (name, c)
    for name in ("slot", "grad", "cam"):
        assert set(result.rows[name]) == {c for n, c in want if n == name}, name
        assert float(result.rows[name]["area"].max()) > 0.0, name
    # the printed line is the formatter's over these values
    assert X.format_row("cam", result.rows["cam"]).startswith("table cam: images 8 area %.6f precision " % result.rows["cam"]["area"].mean())
    # --table_target label explains the labels instead
    args.table_target, args.causal, args.infidelity = "label", False, False
    by_label = X.explanation_table(args, model, batches[:1], ["cam"])
    lab = batches[0]["label"]
    loc = A.localization(K.cam_maps(A.gradcam(model, batches[0]["image"], classes=lab), 64, 64, 0.1), batches[0]["boxes"],
                         batches[0]["n_boxes"])
    assert np.array_equal(by_label.rows["cam"]["area"], loc.area[:, 0].cpu().numpy())
    assert np.array_equal(by_label.correct, (torch.cat(preds)[:4] == lab.cpu()).numpy())
    with pytest.raises(ValueError, match="fccam"):
        X.explanation_table(args, model, batches[:1], ["fccam"])


def test_one_call_on_the_baseline(tmp_path, monkeypatch, capsys):
    from scouter_amd.tools import explanation_table as X
    torch.manual_seed(7)
    monkeypatch.setattr(sys, "argv", ["explanation_table.py"] + MODEL + [
        "--use_slot", "false", "--fccam", "true", "--cam", "true", "--localization", "true", "--output_dir", str(tmp_path / "none")])
    result = X.main()
    rows = _lines(capsys.readouterr().out, ["cam", "fccam"])                # table order; no slot row on the baseline
    for name in ("cam", "fccam"):
        assert list(rows[name]) == ["images", "area", "precision", "pointing", "boxed", "empty"]
        assert rows[name]["images"] == [8.0] and 0.0 <= rows[name]["area"][0] <= 1.0
    assert "slot" not in result.rows and float(result.rows["fccam"]["area"].max()) > 0.0


def test_fccam_on_a_slot_model_is_refused_before_any_work(monkeypatch):
    from scouter_amd import test as T
    from scouter_amd.tools import explanation_table as X
    monkeypatch.setattr(sys, "argv", ["explanation_table.py"] + MODEL + ["--use_slot", "true", "--fccam", "true"])
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    with pytest.raises(ValueError, match="fccam"):
        X.main()
