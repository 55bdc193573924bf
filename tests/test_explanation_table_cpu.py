"""The table tool (scouter_amd/tools/explanation_table.py) without a device: its parser is the single-image tool's plus five
options, the single-image tool's own parser and table are what tests/test_test_tool_cpu.py records, and the host-side pieces --
the boxes file, the seeded synthetic boxes, the means and the printed line, the refusals -- do what the module docstring says."""
import argparse

import numpy as np
import pytest

from scouter_amd import test as T
from scouter_amd.tools import explanation_table as X
from scouter_amd.train import get_args_parser

from test_test_tool_cpu import NAMES, OWN_DEFAULTS

TABLE_DEFAULTS = {"table_images": 64, "table_target": "pred", "fccam": False, "localization": False, "boxes_file": ""}


# ------------------------------------------------------------------------------------------------ the two parsers
def test_the_single_image_tool_is_as_recorded():
    known = vars(get_args_parser().parse_args([]))
    own = {k: v for k, v in vars(T.get_test_parser().parse_args([])).items() if k not in known}
    assert own == OWN_DEFAULTS
    assert len(T.FAMILIES) == 14 and [f.name for f in T.FAMILIES] == NAMES
    assert [s.name for s in T.SCORES] == ["causal", "infidelity", "sensitivity"]
    assert "fccam" not in T._ROWS and "localization" not in T._ROWS


def test_the_table_parser_adds_exactly_five_options():
    base = vars(T.get_test_parser().parse_args([]))
    table = vars(X.get_table_parser().parse_args([]))
    assert {k: v for k, v in table.items() if k not in base} == TABLE_DEFAULTS
    assert {k: table[k] for k in base} == base                              # every inherited option keeps its default
    for k, v in TABLE_DEFAULTS.items():
        assert type(table[k]) is type(v), k
    a = X.get_table_parser().parse_args(["--table_images", "8", "--table_target", "label", "--fccam", "true", "--localization",
                                         "true", "--boxes_file", "b.txt", "--rise_masks", "6", "--cam", "true"])
    assert (a.table_images, a.table_target, a.fccam, a.localization, a.boxes_file) == (8, "label", True, True, "b.txt")
    assert a.rise_masks == 6 and a.cam is True
    with pytest.raises(SystemExit):
        X.get_table_parser().parse_args(["--table_target", "both"])


def test_the_table_extends_the_families_by_one_row():
    assert [f.name for f in X.FAMILIES] == NAMES + ["fccam"]
    assert X.FAMILIES[:14] == T.FAMILIES
    row = T._row("fccam", X._ROWS)
    assert (row.explain, row.maps, row.options, row.reduce, row.flag) == ("fccam", "fccam_maps", (), None, True)
    with pytest.raises(ValueError, match="fccam"):
        T._row("fccam")                                                     # the single-image tool does not know it
    assert T.option_kwargs(argparse.Namespace(), "fccam", X._ROWS) == {}
    assert T.option_kwargs(argparse.Namespace(rise_masks=6), "rise", X._ROWS) == dict(n_masks=6, batch=250)


def test_the_chosen_families_come_in_table_order():
    parse = X.get_table_parser().parse_args
    assert X.chosen_families(parse(["--rise", "true", "--cam", "true", "--grad", "true"])) == ["slot", "grad", "cam", "rise"]
    assert X.chosen_families(parse(["--use_slot", "false", "--fccam", "true", "--cam", "true"])) == ["cam", "fccam"]
    assert X.chosen_families(parse(["--use_slot", "false"])) == []


# ------------------------------------------------------------------------------------------------ refusals
def test_sensitivity_is_refused():
    args = X.get_table_parser().parse_args(["--sensitivity", "true", "--cam", "true"])
    with pytest.raises(ValueError, match="sensitivity"):
        X.check_request(X.chosen_families(args), args.use_slot, args.sensitivity)
    X.check_request(["slot", "cam"], True, False)


def test_fccam_on_a_slot_model_and_slot_on_the_baseline_are_refused(monkeypatch):
    with pytest.raises(ValueError, match="fccam.*use_slot false"):
        X.check_request(["slot", "fccam"], True)
    with pytest.raises(ValueError, match="slot"):
        X.check_request(["slot", "cam"], False)
    with pytest.raises(ValueError, match="nope"):
        X.check_request(["nope"], True)
    X.check_request(["cam", "fccam"], False)
    # main() refuses before it builds a model
    import sys
    monkeypatch.setattr(sys, "argv", ["explanation_table.py", "--fccam", "true", "--use_slot", "true"])
    monkeypatch.setattr(T, "build_model", lambda args: pytest.fail("a model was built"))
    with pytest.raises(ValueError, match="fccam"):
        X.main()


# ------------------------------------------------------------------------------------------------ the boxes
def test_the_boxes_file(tmp_path):
    path = tmp_path / "boxes.txt"
    path.write_text("a 0.25 0.5 0.75 1.0\n\nb 0 0 1 1\na 0.3 0.3 0.7 0.7\n")
    table = X.read_boxes_file(str(path))
    assert table == {"a": [(0.25, 0.5, 0.75, 1.0), (0.3, 0.3, 0.7, 0.7)], "b": [(0.0, 0.0, 1.0, 1.0)]}
    # on a pixel edge: floor and ceil leave it; off one: the box grows to the pixels it touches
    assert X.box_pixels((0.25, 0.5, 0.75, 1.0), 64, 64) == (16, 32, 48, 64)
    assert X.box_pixels((0.3, 0.3, 0.7, 0.7), 64, 32) == (9, 19, 23, 45)       # (x against W = 32, y against H = 64)
    assert X.box_pixels((0.26, 0.51, 0.74, 0.99), 64, 64) == (16, 32, 48, 64)
    assert X.box_pixels((0.0, 0.0, 1.0, 1.0), 7, 9) == (0, 0, 9, 7)
    boxes, n = X.named_boxes(["a", "zzz", "b"], table, 64, 64)
    assert boxes.dtype == np.int32 and n.dtype == np.int32 and boxes.shape == (3, 2, 4)
    assert n.tolist() == [2, 0, 1]                                          # an unknown name has no box
    assert boxes[0].tolist() == [[16, 32, 48, 64], [19, 19, 45, 45]] and boxes[2, 0].tolist() == [0, 0, 64, 64]
    assert not boxes[1].any()
    none, n0 = X.named_boxes(["q"], table, 8, 8)
    assert none.shape == (1, 1, 4) and n0.tolist() == [0]


@pytest.mark.parametrize("bad", ["a 0.1 0.2 0.3", "a 0.1 0.2 0.3 x", "a 0.1 0.2 0.3 0.4 0.5", "a 0.1 0.2 0.3 nan"])
def test_a_malformed_line_names_itself(tmp_path, bad):
    path = tmp_path / "boxes.txt"
    path.write_text("ok 0 0 1 1\n" + bad + "\n")
    with pytest.raises(ValueError, match="line 2") as err:
        X.read_boxes_file(str(path))
    assert bad in str(err.value)


def test_too_many_boxes_are_refused():
    X.batch_boxes([[(0, 0, 1, 1)] * 32])
    with pytest.raises(ValueError, match="33"):
        X.batch_boxes([[(0, 0, 1, 1)] * 33])


def test_the_synthetic_boxes_are_seeded():
    a = [X.synthetic_box(i, 64, 64) for i in range(16)]
    assert a == [X.synthetic_box(i, 64, 64) for i in range(16)]
    assert len(set(a)) == 16
    for x0, y0, x1, y1 in a:
        assert 0 <= x0 < x1 <= 64 and 0 <= y0 < y1 <= 64 and x1 - x0 >= 16 and y1 - y0 >= 16
    u = np.random.default_rng(5).random(4)
    assert X.synthetic_box(5, 100, 200) == X.box_pixels((0.5 * u[0], 0.5 * u[1], 0.5 * u[0] + 0.25 + 0.25 * u[2],
                                                         0.5 * u[1] + 0.25 + 0.25 * u[3]), 100, 200)


# ------------------------------------------------------------------------------------------------ the means and the line
COLS = {"area": np.array([0.25, 0.5, 0.75, 1.0]), "ratio": np.array([0.1, 0.1, 0.1, 0.1]),
        "precision": np.array([0.5, 0.9, 0.0, 0.25]), "pointing": np.array([1.0, 1.0, 0.0, 0.0]),
        "boxed": np.array([1.0, 0.0, 1.0, 1.0]), "empty": np.array([0.0, 0.0, 1.0, 0.0]),
        "deletion": np.array([0.1, 0.2, 0.3, 0.4]), "insertion": np.array([0.5, 0.5, 0.5, 0.5]),
        "infidelity_raw": np.array([1.0, 2.0, 3.0, 4.0]), "infidelity_normalized": np.array([0.5, 0.5, 1.5, 1.5])}


def test_precision_and_pointing_leave_out_the_unboxed_and_the_empty():
    m = X.column_means(COLS)
    assert m["precision"] == np.array([0.5, 0.25]).mean() and m["pointing"] == 0.5      # images 0 and 3
    assert m["boxed"] == 3 and m["empty"] == 1 and m["area"] == 0.625 and m["deletion"] == COLS["deletion"].mean()
    none = X.column_means(dict(COLS, boxed=np.zeros(4)))
    assert np.isnan(none["precision"]) and np.isnan(none["pointing"])


def test_the_line_holds_only_the_columns_asked_for_in_order():
    assert X.format_row("slot", COLS) == (
        "table slot: images 4 area 0.625000 ratio 0.100000 precision 0.375000 pointing 0.500000 boxed 3 empty 1 "
        "deletion 0.250000 insertion 0.500000 infidelity 2.500000e+00 1.000000e+00")
    loc = {k: COLS[k] for k in ("empty", "boxed", "pointing", "precision", "area")}     # given in any order
    assert X.format_row("cam", loc) == "table cam: images 4 area 0.625000 precision 0.375000 pointing 0.500000 boxed 3 empty 1"
    assert X.format_row("rise", {"insertion": COLS["insertion"], "deletion": COLS["deletion"]}) == \
        "table rise: images 4 deletion 0.250000 insertion 0.500000"
    assert X.format_row("grad", {k: COLS[k] for k in ("infidelity_raw", "infidelity_normalized")}) == \
        "table grad: images 4 infidelity 2.500000e+00 1.000000e+00"
    assert X.format_row("cam", {}, images=8) == "table cam: images 8"
