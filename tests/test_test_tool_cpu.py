"""The single-image tool (scouter_amd/test.py) states every explanation family once, in FAMILIES, and every score once, in
SCORES; the parser, the option-to-keyword function and the run_<name> functions are derived from those rows.  These tests need
no device: the parser as a whole against a recorded literal, one row per family in the documented order, the table's defaults
against the signatures of tools/attribution.py, and the refusal of an unknown family."""
import argparse
import inspect

import pytest

from scouter_amd import test as T
from scouter_amd.tools import attribution as A
from scouter_amd.train import get_args_parser

NAMES = ["slot", "grad", "cam", "rise", "scorecam", "ig", "smoothgrad", "campp", "smoothcampp", "extremal", "iba", "igos", "sscam",
         "iscam"]

# every option of get_test_parser() that train.py's parser does not know, with its default: recorded from the parser as it
# stood before the table, when every add_argument line was written out by hand
OWN_DEFAULTS = {
    "checkpoint": "", "image": "", "label": None, "vis_dir": "sloter/vis",
    "cam": False,
    "rise": False, "rise_masks": 4000, "rise_batch": 250,
    "causal": False, "causal_step": 0,
    "scorecam": False, "scorecam_batch": 250,
    "ig": False, "ig_steps": 50, "ig_batch": 50,
    "smoothgrad": False, "smoothgrad_samples": 50, "smoothgrad_sigma": 1.0, "smoothgrad_batch": 50,
    "campp": False,
    "smoothcampp": False, "smoothcampp_samples": 4, "smoothcampp_sigma": 0.3, "smoothcampp_batch": 4,
    "extremal": False, "extremal_area": 0.1, "extremal_iters": 800, "extremal_variant": "preserve", "extremal_batch": 50,
    "iba": False, "iba_beta": 10.0, "iba_steps": 10, "iba_samples_per_step": 10, "iba_sigma": 1.0, "iba_fit": 5000, "iba_batch": 0,
    "igos": False, "igos_size": 8, "igos_iters": 15, "igos_steps": 20, "igos_l1": 1.0, "igos_tv": 20.0, "igos_batch": 50,
    "sscam": False, "sscam_samples": 35, "sscam_sigma": 2.0, "sscam_batch": 250,
    "iscam": False, "iscam_samples": 10, "iscam_batch": 250,
    "infidelity": False, "infidelity_samples": 50, "infidelity_sigma": 0.003, "infidelity_batch": 50,
    "sensitivity": False, "sensitivity_samples": 10, "sensitivity_radius": 0.02, "sensitivity_batch": 11,
}

# one value that is not the default for each of them, as the command line spells it and as the parser must read it
OTHER = {
    "checkpoint": ("a.pth", "a.pth"), "image": ("b.jpg", "b.jpg"), "label": ("3", 3), "vis_dir": ("out", "out"),
    "cam": ("true", True),
    "rise": ("true", True), "rise_masks": ("6", 6), "rise_batch": ("4", 4),
    "causal": ("true", True), "causal_step": ("64", 64),
    "scorecam": ("true", True), "scorecam_batch": ("7", 7),
    "ig": ("true", True), "ig_steps": ("3", 3), "ig_batch": ("2", 2),
    "smoothgrad": ("true", True), "smoothgrad_samples": ("3", 3), "smoothgrad_sigma": ("0.5", 0.5), "smoothgrad_batch": ("2", 2),
    "campp": ("true", True),
    "smoothcampp": ("true", True), "smoothcampp_samples": ("2", 2), "smoothcampp_sigma": ("0.25", 0.25), "smoothcampp_batch": ("3", 3),
    "extremal": ("true", True), "extremal_area": ("0.25", 0.25), "extremal_iters": ("2", 2), "extremal_variant": ("delete", "delete"),
    "extremal_batch": ("5", 5),
    "iba": ("true", True), "iba_beta": ("2.5", 2.5), "iba_steps": ("2", 2), "iba_samples_per_step": ("3", 3), "iba_sigma": ("0", 0.0),
    "iba_fit": ("8", 8), "iba_batch": ("4", 4),
    "igos": ("true", True), "igos_size": ("4", 4), "igos_iters": ("1", 1), "igos_steps": ("2", 2), "igos_l1": ("0.5", 0.5),
    "igos_tv": ("2.0", 2.0), "igos_batch": ("7", 7),
    "sscam": ("true", True), "sscam_samples": ("2", 2), "sscam_sigma": ("0.5", 0.5), "sscam_batch": ("256", 256),
    "iscam": ("true", True), "iscam_samples": ("2", 2), "iscam_batch": ("256", 256),
    "infidelity": ("true", True), "infidelity_samples": ("3", 3), "infidelity_sigma": ("0.01", 0.01), "infidelity_batch": ("2", 2),
    "sensitivity": ("true", True), "sensitivity_samples": ("2", 2), "sensitivity_radius": ("0.05", 0.05), "sensitivity_batch": ("3", 3),
}

# the tools/attribution.py function whose signature states a row's defaults, where the row's `explain` hands them on as **kwargs
SIGNATURE = {"extremal": "extremal_perturbation", "igos": "igos", "causal": "causal_metrics", "infidelity": "infidelity",
             "sensitivity": "sensitivity_max"}


# ------------------------------------------------------------------------------------------------ the parser as a whole
def test_the_parser_adds_exactly_the_recorded_options_and_defaults():
    known = vars(get_args_parser().parse_args([]))
    own = {k: v for k, v in vars(T.get_test_parser().parse_args([])).items() if k not in known}
    assert own == OWN_DEFAULTS
    for k, v in own.items():
        assert type(v) is type(OWN_DEFAULTS[k]), k


def test_every_option_parses_a_value_of_its_type():
    assert set(OTHER) == set(OWN_DEFAULTS)
    argv = [w for k, (text, _) in OTHER.items() for w in ("--" + k, text)]
    a = T.get_test_parser().parse_args(argv)
    for k, (_, want) in OTHER.items():
        got = getattr(a, k)
        assert got == want and type(got) is type(want) and want != OWN_DEFAULTS[k], k


def test_a_variant_outside_the_choices_exits():
    with pytest.raises(SystemExit):
        T.get_test_parser().parse_args(["--extremal_variant", "bogus"])


# ------------------------------------------------------------------------------------------------ one row per family
def test_the_table_names_the_fourteen_families_in_order():
    assert [f.name for f in T.FAMILIES] == NAMES
    assert [s.name for s in T.SCORES] == ["causal", "infidelity", "sensitivity"]
    for name in NAMES[1:]:
        assert callable(getattr(T, "run_" + name)), name
    assert not hasattr(T, "run_slot")
    assert callable(T.run_family)


def test_an_empty_namespace_gets_the_parsers_defaults():
    parsed, empty = T.get_test_parser().parse_args([]), argparse.Namespace()
    for row in T.FAMILIES + T.SCORES:
        assert T.option_kwargs(empty, row.name) == T.option_kwargs(parsed, row.name), row.name
        for o in row.options:                                              # and the table's default IS the parser's
            assert getattr(parsed, "%s_%s" % (row.name, o.suffix)) == o.default, (row.name, o.suffix)
    assert T.option_kwargs(empty, "cam") == {} and T.option_kwargs(empty, "slot") == {}
    assert T.option_kwargs(empty, "rise") == dict(n_masks=4000, batch=250)
    given = argparse.Namespace(rise_masks=6, sscam_sigma=0.5)               # what is there is read, the rest defaulted
    assert T.option_kwargs(given, "rise") == dict(n_masks=6, batch=250)
    assert T.option_kwargs(given, "sscam") == dict(n_samples=35, sigma=0.5, batch=250)


# ------------------------------------------------------------------------------------------------ defaults against the library
def test_the_tables_defaults_are_the_librarys():
    checked = []
    for row in T.FAMILIES + T.SCORES:
        if not row.options:
            continue
        sig = inspect.signature(getattr(A, SIGNATURE.get(row.name) or row.explain)).parameters
        for o in row.options:
            if o.keyword is None or o.convert is not None:
                continue
            assert o.keyword in sig, (row.name, o.keyword)
            assert sig[o.keyword].default == o.default and type(sig[o.keyword].default) is o.type, (row.name, o.keyword)
            checked.append("%s_%s" % (row.name, o.suffix))
    # every option but the four converted ones and --iba_fit, which feeds iba_estimate
    assert sorted(checked) == sorted(k for k in OWN_DEFAULTS if "_" in k and k not in (
        "vis_dir", "extremal_area", "iba_sigma", "iba_batch", "iba_fit", "causal_step"))
    assert inspect.signature(A.iba_estimate).parameters["n_samples"].default == 5000
    # the maps functions that restate the defaults agree as well
    for name in ("scorecam", "sscam", "iscam"):
        maps, flt = (inspect.signature(getattr(A, n)).parameters for n in (name + "_maps", name))
        for o in T._row(name).options:
            assert maps[o.keyword].default == flt[o.keyword].default, (name, o.keyword)


def test_the_converted_options():
    empty = argparse.Namespace()
    sig = inspect.signature(A.extremal_perturbation).parameters
    assert T.option_kwargs(empty, "extremal")["areas"] == (0.1,) == sig["areas"].default
    assert T.option_kwargs(argparse.Namespace(extremal_area=0.25), "extremal")["areas"] == (0.25,)
    sig = inspect.signature(A.information_bottleneck).parameters
    assert T.option_kwargs(empty, "iba")["sigma"] == 1.0 == sig["sigma"].default
    assert T.option_kwargs(empty, "iba")["batch"] is None and sig["batch"].default is None
    zero = T.option_kwargs(argparse.Namespace(iba_sigma=0.0, iba_batch=0), "iba")
    assert zero["sigma"] is None and zero["batch"] is None
    some = T.option_kwargs(argparse.Namespace(iba_sigma=2.0, iba_batch=8), "iba")
    assert some["sigma"] == 2.0 and some["batch"] == 8
    assert "fit" not in T.option_kwargs(empty, "iba") and "n_samples" not in T.option_kwargs(empty, "iba")
    assert T.option_kwargs(empty, "causal") == dict(step=None) and inspect.signature(A.causal_metrics).parameters["step"].default is None
    assert T.option_kwargs(argparse.Namespace(causal_step=64), "causal") == dict(step=64)


# ------------------------------------------------------------------------------------------------ unknown names
def test_an_unknown_family_raises():
    args = argparse.Namespace()
    with pytest.raises(ValueError, match="nope"):
        T._family_attribution(args, None, None, 0, family="nope")
    with pytest.raises(ValueError, match="nope"):
        T.run_family(args, None, None, "unused", "nope")
    with pytest.raises(ValueError, match="nope"):
        T.option_kwargs(args, "nope")
    assert T._family_attribution(args, None, None, 0, family="slot", slot_map="given") == "given"
