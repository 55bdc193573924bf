"""The single-image tool with every family and every score on (-m gpu): one scouter_amd.test main() call at the smallest
settings that still take every branch of every row of its table.  What each family draws and each score computes is checked
where the family was added (tests/test_*_gpu.py); this test is about the table: every row is drawn, and every score names every
row in the table's order."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

NAMES = ["slot", "grad", "cam", "rise", "scorecam", "ig", "smoothgrad", "campp", "smoothcampp", "extremal", "iba", "igos", "sscam",
         "iscam"]


def test_every_family_and_every_score_in_one_call(tmp_path, monkeypatch, capsys):
    """--img_size 96: at 64 the window of --iba does not fit the 2 x 2 feature map; --causal_step 4608 gives 3 points a curve"""
    from PIL import Image
    from scouter_amd import test as T
    assert [f.name for f in T.FAMILIES] == NAMES
    vis = tmp_path / "vis"
    monkeypatch.setattr(sys, "argv", [
        "test.py", "--model", "resnet18", "--dataset", "MNIST", "--channel", "512", "--num_classes", "10", "--slots_per_class", "1",
        "--to_k_layer", "1", "--power", "1", "--use_slot", "true", "--pre_trained", "false", "--img_size", "96",
        "--synthetic_data", "true", "--synthetic_len", "32", "--batch_size", "8", "--num_workers", "0",
        "--grad", "true", "--cam", "true", "--rise", "true", "--rise_masks", "6", "--rise_batch", "4",
        "--scorecam", "true", "--scorecam_batch", "256", "--ig", "true", "--ig_steps", "3", "--ig_batch", "2",
        "--smoothgrad", "true", "--smoothgrad_samples", "3", "--smoothgrad_batch", "2", "--campp", "true",
        "--smoothcampp", "true", "--smoothcampp_samples", "2", "--smoothcampp_batch", "2", "--extremal", "true", "--extremal_iters", "2",
        "--iba", "true", "--iba_steps", "2", "--iba_samples_per_step", "2", "--iba_fit", "8", "--iba_batch", "8",
        "--igos", "true", "--igos_size", "4", "--igos_iters", "1", "--igos_steps", "2",
        "--sscam", "true", "--sscam_samples", "2", "--sscam_batch", "256", "--iscam", "true", "--iscam_samples", "2", "--iscam_batch", "256",
        "--causal", "true", "--causal_step", "4608", "--infidelity", "true", "--infidelity_samples", "3", "--infidelity_batch", "2",
        "--sensitivity", "true", "--sensitivity_samples", "2", "--sensitivity_batch", "3",
        "--vis_dir", str(vis), "--output_dir", str(tmp_path / "none")])
    T.main()
    text = capsys.readouterr().out.splitlines()
    for name in NAMES:
        for c in range(10):
            png = Image.open(vis / ("%s_%d.png" % (name, c)))
            assert png.mode == "L" and (name == "slot" or png.size == (96, 96)), (name, c)
        assert not os.path.exists(vis / ("%s_10.png" % name)), name
    assert len(os.listdir(vis)) == 10 * len(NAMES)
    # the number of values each score prints after `<score> <family> class <c>:`, every second word from the fifth on
    classes = set()
    for score, n_values in (("causal", 2), ("infidelity", 3), ("sensitivity", 1)):
        lines = [ln.split() for ln in text if ln.startswith(score + " ")]
        assert [ln[1] for ln in lines] == NAMES, score
        for ln in lines:
            assert ln[2] == "class" and ln[3].endswith(":") and len(ln) == 4 + 2 * n_values, ln
            classes.add(int(ln[3][:-1]))
            assert all(math.isfinite(float(v)) for v in ln[5::2]), ln
    assert len(classes) == 1 and text[-1] == "%d" % classes.pop()         # one shared class: the prediction main() prints last
