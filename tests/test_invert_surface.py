"""The surface of dsurftomo_amd/invert.py that callers and scripts depend on, pinned by literals recorded before the analyses moved into
dsurftomo_amd/analyses: main()'s flags, run()'s keywords and defaults, the refusal of an unknown keyword, and the bytes of the five
"one row per member" files, which one table-driven writer (io.write_table) now produces.  No GPU."""
import argparse
import inspect

import pytest

from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei

FLAGS = ['--azimuthal', '--azimuthal-damp', '--azimuthal-weight', '--bootstrap', '--bootstrap-seed', '--checkerboard', '--crossval', '--crossval-by',
         '--crossval-damps', '--crossval-iter', '--crossval-nonlinear', '--crossval-seed', '--crossval-weights', '--help', '--host-rows', '--line-search',
         '--maxiter', '--out', '--resolution', '--tradeoff-damps', '--tradeoff-iter', '--tradeoff-nonlinear', '--tradeoff-weights', '--voronoi',
         '--voronoi-damp', '--voronoi-seed', '--voronoi-update', '--voronoi-zscale', '-h']

RUN_DEFAULTS = {'maxiter': None, 'out_dir': '.', 'log': print, 'seed': 1, 'host_rows': False, 'bootstrap': 0, 'bootstrap_seed': 1, 'resolution': False,
                'checkerboard': (), 'resolution_chunk': None, 'tradeoff_weights': None, 'tradeoff_damps': None, 'tradeoff_iter': 1, 'tradeoff_chunk': None,
                'voronoi': None, 'voronoi_seed': 1, 'voronoi_zscale': 1.0, 'voronoi_damp': None, 'voronoi_update': False, 'voronoi_chunk': None,
                'crossval': None, 'crossval_weights': None, 'crossval_damps': None, 'crossval_by': 'datum', 'crossval_seed': 1, 'crossval_iter': 1,
                'crossval_chunk': None, 'line_search': None, 'tradeoff_nonlinear': False, 'crossval_nonlinear': False, 'azimuthal': False,
                'azimuthal_weight': None, 'azimuthal_damp': None}


@pytest.fixture()
def parser(monkeypatch):
    """main()'s parser, caught at parse_args"""
    caught = []

    def grab(self, argv=None):
        caught.append(self)
        raise SystemExit(0)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", grab)
    with pytest.raises(SystemExit):
        invert.main(["x"])
    monkeypatch.undo()
    return caught[0]


def test_the_flags_of_main(parser):
    assert sorted(s for a in parser._actions for s in a.option_strings) == FLAGS


def test_help_names_every_flag_and_describes_every_analysis(parser):
    text = parser.format_help()
    for flag in FLAGS:
        assert flag in text
    # the first words of each analysis's paragraph of the description, which the modules' docstrings now carry
    for start in ("--bootstrap R (R >= 2) adds", "--resolution and --checkerboard NX,NY,NZ add", "--tradeoff-weights W1,W2,... adds", "--voronoi K,NCELLS adds",
                  "--crossval NFOLDS (>= 2) with --crossval-weights adds", "--line-search A1,A2,... (finite, each >= 0", "--tradeoff-nonlinear (with --tradeoff-weights)",
                  "--azimuthal adds one joint step"):
        assert start in text


def test_the_flags_defaults_are_the_keywords_defaults(parser):
    """a flag's destination is run()'s keyword and parses to its default (--checkerboard: argparse appends to a list, run() takes any sequence)"""
    args = vars(parser.parse_args(["x"]))
    for dest in set(args) - {"directory", "maxiter", "out", "host_rows"}:
        assert args[dest] == RUN_DEFAULTS[dest] or (dest == "checkerboard" and args[dest] == [])
    assert set(RUN_DEFAULTS) - set(args) == {"out_dir", "log", "seed", "resolution_chunk", "tradeoff_chunk", "voronoi_chunk", "crossval_chunk"}


def test_the_keywords_and_defaults_of_run():
    sig = inspect.signature(invert.run)
    named = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert list(sig.parameters)[0] == "directory" and list(sig.parameters)[:7] == ["directory", "maxiter", "out_dir", "log", "seed", "host_rows", "options"]
    assert dict(named, **invert.check_options({}, False, None)) == RUN_DEFAULTS
    assert invert.check_options(dict(bootstrap=8, voronoi_chunk=128), False, None)["bootstrap"] == 8


def test_run_refuses_an_unknown_keyword_before_the_library(monkeypatch, tmp_path):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(TypeError, match="no_such_option"):
        invert.run(str(tmp_path), no_such_option=1)
    with pytest.raises(TypeError, match="no_such_plan"):
        invert.iteration_device(None, None, None, None, print, no_such_plan=1)


ROWS = [   # (writer, reader, one row, the line the writer wrote before the table-driven one, the header line before it)
    (invert.write_tradeoff, invert.read_tradeoff,
     dict(weight=0.1, damp=2.5, misfit=1.0 / 3, rough=2e-7, xnorm=123456.789, itn=17, istop=2, dv_min=-0.30000001192092896, dv_max=0.25),
     "0.1 2.5 0.33333333333333331 1.9999999999999999e-07 123456.789 17 2 -0.300000012 0.25\n", ""),
    (invert.write_crossval, invert.read_crossval,
     dict(weight=0.1, damp=2.5, cv_rms=1.0 / 3, cv_se=2e-7, train_rms=0.7, misfit=12.5, rough=1e-3, xnorm=123456.789, itn_min=3, itn_max=400),
     "0.1 2.5 0.33333333333333331 1.9999999999999999e-07 0.69999999999999996 12.5 0.001 123456.789 3 400\n", ""),
    (taipei.write_tradeoff_nonlinear, taipei.read_tradeoff_nonlinear,
     dict(weight=0.1, damp=2.5, predicted_rms=1.0 / 3, weighted_rms=0.7, rms=2e-7, disp_failures=3),
     "0.10000000000000001 2.5 0.33333333333333331 0.69999999999999996 1.9999999999999999e-07 3\n", "# weight damp predicted_rms weighted_rms rms disp_failures\n"),
    (taipei.write_crossval_nonlinear, taipei.read_crossval_nonlinear,
     dict(weight=0.1, damp=2.5, heldout_rms=1.0 / 3, full_rms=0.7, cv_rms=2e-7, disp_failures=0),
     "0.10000000000000001 2.5 0.33333333333333331 0.69999999999999996 1.9999999999999999e-07 0\n", "# weight damp heldout_rms full_rms cv_rms disp_failures\n"),
    (taipei.write_line_search, taipei.read_line_search,
     dict(iteration=2, alpha=0.5, weighted_rms=1.0 / 3, rms=0.7, disp_failures=0, chosen=True),
     "   2 0.5 0.33333333333333331 0.69999999999999996 0 1\n", "# iteration alpha weighted_rms rms disp_failures chosen\n"),
]


@pytest.mark.parametrize("write, read, row, line, header", ROWS, ids=["tradeoff", "crossval", "tradeoff_nonlinear", "crossval_nonlinear", "line_search"])
def test_the_table_files_keep_their_bytes(tmp_path, write, read, row, line, header):
    path = str(tmp_path / "table.dat")
    write(path, [row, row])
    with open(path) as fh:
        assert fh.read() == header + line + line
    back = read(path)
    assert len(back) == 2 and list(back[0]) == list(row)
    for k, v in row.items():
        # the float32 columns of Tradeoff.dat / Crossval.dat come back as the float32 value their 9 digits round to, everything else exactly
        assert back[1][k] == v or (write in (invert.write_tradeoff, invert.write_crossval) and k in ("weight", "damp") and abs(back[1][k] - v) < 1e-8)
